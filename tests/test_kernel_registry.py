"""A kernel form is declared where it is launched: the launch helpers of dsd_internal.h register every kernel instantiation they
are instantiated with while the library is loaded, and the create functions raise the dynamic-LDS limit of exactly those
(prepare_kernels, api.hip).  So "can be launched" implies "has been prepared", with no second list to keep in step.  Checked
here without a GPU: a stand-alone program prints the registry of the built library, and per kernel group it must hold the
kernel instantiations the compiler emits for that group's files - no more (nothing is prepared that cannot be launched, and
no family touches another's code objects), no fewer (a kernel launched past the helpers would miss its limit)."""
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "diffsinger_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tools"))

# KernelGroup of dsd_internal.h -> the files whose kernels carry it
GROUPS = {
    1: ["gemm.hip"],
    2: ["wn_layer.hip", "wn_layer_x3.hip", "wn_rowsplit.hip", "wn_rows.hip", "wn_edge.hip"],
    4: ["lynx_layer.hip", "lynx_x3.hip"],
    8: ["tconv.hip", "voc_x3.hip", "vocoder_kernels.hip"],
}
# vocoder_kernels.hip: only the noise conv asks for more than the default 64 KiB of dynamic LDS
ONLY = {"vocoder_kernels.hip": "voc_noise_conv_kernel"}

PROGRAM = r"""
#include <dlfcn.h>
#include <cstdio>
namespace dsd { int kernel_registry_get(int i, const void** host_stub, int* group); }
int main() {
    const void* stub = nullptr;
    int group = 0, i = 0;
    for (; dsd::kernel_registry_get(i, &stub, &group); ++i) {
        Dl_info info;
        const bool named = dladdr(stub, &info) && info.dli_sname && info.dli_saddr == stub;
        printf("%d %s\n", group, named ? info.dli_sname : "?");
    }
    return i > 0 ? 0 : 1;
}
"""


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(names)
    # the host stub of kernel K is dsd::__device_stub__K: the same template arguments and parameter list
    return [re.sub(r"\s*\[clone [^\]]*\]", "", n.replace("__device_stub__", "")).strip() for n in out]


@pytest.fixture(scope="module")
def registry(tmp_path_factory):
    from diffsinger_amd import _lib
    tmp = tmp_path_factory.mktemp("registry")
    src, exe = tmp / "registry.cpp", tmp / "registry"
    src.write_text(PROGRAM)
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.run(["g++", "-std=c++17", "-Wall", str(src), "-L" + libdir, "-ldsdenoise", "-L/opt/rocm/lib", "-lamdhip64", "-ldl",
                    "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)      # needs no device: nothing calls HIP
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    rows = [line.split(" ", 1) for line in r.stdout.splitlines()]
    names = demangle([n for _, n in rows])
    reg = {}
    for (g, _), n in zip(rows, names):
        reg.setdefault(int(g), []).append(n)
    return reg


@pytest.fixture(scope="module")
def compiled():
    """file -> demangled names of the kernel instantiations hipcc emits for it (tools/check_resources.py)"""
    import check_resources
    files = [f for fs in GROUPS.values() for f in fs]
    with ThreadPoolExecutor(max_workers=min(len(files), os.cpu_count() or 1, 16)) as pool:
        found = list(pool.map(lambda f: check_resources.analyse(os.path.join(CSRC, f)), files))
    return {f: demangle([k["name"] for k in ks]) for f, ks in zip(files, found)}


def test_registry_holds_each_groups_kernels_and_no_others(registry, compiled):
    assert sorted(registry) == sorted(GROUPS), "a kernel is registered under an unknown group"
    for group, files in GROUPS.items():
        want = []
        for f in files:
            names = compiled[f]
            assert names, f
            if f in ONLY:
                names = [n for n in names if ONLY[f] in n]
                assert names, f
            want += names
        got = registry[group]
        assert len(got) == len(set(got)), f"group {group}: a kernel is registered twice"
        assert len(want) == len(set(want))
        assert len(got) == len(want), (f"group {group}: {len(got)} kernels registered, {len(want)} compiled; "
                                       f"only registered {sorted(set(got) - set(want))[:8]}, "
                                       f"only compiled {sorted(set(want) - set(got))[:8]}")
        if "?" not in got:      # dladdr names every host stub: compare the instantiations themselves
            assert sorted(got) == sorted(want)


def test_the_limit_is_raised_in_one_place():
    """No hand-kept set-up is left beside the registry: no launcher flag, no per-file init list, and the attribute call stands
    in the one preparer."""
    hits = {"attr_done": [], "_init_all(": [], "hipFuncAttributeMaxDynamicSharedMemorySize": []}
    sources = sorted(fn for fn in os.listdir(CSRC) if fn.endswith((".hip", ".h")))
    assert "api.hip" in sources and "gemm.hip" in sources and "dsd_internal.h" in sources
    for fn in sources:
        text = open(os.path.join(CSRC, fn)).read()
        for word in hits:
            hits[word] += [fn] * text.count(word)
    assert hits["attr_done"] == []
    assert hits["_init_all("] == []
    assert hits["hipFuncAttributeMaxDynamicSharedMemorySize"] == ["api.hip"]
    api = open(os.path.join(CSRC, "api.hip")).read()
    body = api[api.index("int prepare_kernels("):]
    body = body[:body.index("\n}\n")]
    assert "hipFuncAttributeMaxDynamicSharedMemorySize" in body


def test_launch_ledger_lists_the_registry(registry):
    """dsd_kernel_ledger (the launch counts tests/test_gpu_kernel_ledger.py reads): one entry per registry entry, in the
    registry's order and under its group, every name resolved inside the library (dladdr) to the instantiation the
    stand-alone program names; nothing has been launched, so every count is zero, and stays zero over a reset."""
    from diffsinger_amd import _lib
    rows = _lib.kernel_ledger()
    assert len(rows) == sum(len(v) for v in registry.values()) > 0
    assert all(sym for sym, _, _ in rows), [r for r in rows if not r[0]][:8]
    names = demangle([sym for sym, _, _ in rows])
    assert len(set(names)) == len(names)
    odd = [n for n in names if not re.fullmatch(r"(void )?dsd::\w+(<.*>)?\(.*\)", n)]       # a kernel, not some other symbol
    assert not odd, odd[:8]
    got = {}
    for (_, group, _), n in zip(rows, names):
        got.setdefault(group, []).append(n)
    assert got == registry
    assert [c for _, _, c in rows] == [0] * len(rows)
    _lib.kernel_ledger_reset()
    assert _lib.kernel_ledger() == rows


def test_launch_ledger_argument_checks():
    """max_entries = 0 sizes the array; a short array is filled as far as it goes and the count is still the whole
    ledger's; the mistakes a caller can make are DSD_EINVAL."""
    import ctypes as C
    from diffsinger_amd import _lib
    lib, n, m = _lib.lib(), C.c_int32(-1), C.c_int32(-1)
    assert lib.dsd_kernel_ledger(None, 0, C.byref(n)) == 0 and n.value > 3
    rows = (_lib.DsdKernelLaunches * 3)()
    rows[2].group = -7
    assert lib.dsd_kernel_ledger(rows, 2, C.byref(m)) == 0 and m.value == n.value
    assert rows[0].symbol and rows[1].symbol and rows[2].group == -7
    assert [(r[0].encode(), r[1]) for r in _lib.kernel_ledger()[:2]] == [(r.symbol, r.group) for r in rows[:2]]
    assert lib.dsd_kernel_ledger(rows, 3, None) == _lib.DSD_EINVAL
    assert lib.dsd_kernel_ledger(None, 3, C.byref(m)) == _lib.DSD_EINVAL
    assert lib.dsd_kernel_ledger(rows, -1, C.byref(m)) == _lib.DSD_EINVAL
