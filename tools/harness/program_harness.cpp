// Stand-alone memory check of the program builder (diffsinger_amd/csrc/program_api.hip is host code only): builds and
// frees every case of the grid of tests/test_cprogram_host.py and every refused case, under the host compiler's address
// and undefined-behaviour sanitizers.  Not a test of the values (the pytest file holds them against schedule.py): what
// this looks for is a read past the tables, a write past the evaluations, a leak, an overflow on the way.  Host only -
// never loaded into Python, needs no GPU:
//
// (one command line)
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude
//       tools/harness/program_harness.cpp -x c++ diffsinger_amd/csrc/program_api.hip -o /tmp/program_harness
//   /tmp/program_harness            # prints the number of programs built and refused; exit status 0 = clean
//
// The library proper takes dsd::fail and dsd_last_error from api.hip; this program brings its own.
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "dsdenoise.h"

struct dsd_handle;
static std::string g_error;
namespace dsd {
int fail(dsd_handle*, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_error = buf;
    return code;
}
}  // namespace dsd
extern "C" const char* dsd_last_error(const dsd_handle*) { return g_error.c_str(); }

static int g_built = 0, g_refused = 0, g_bad = 0;

static dsd_sampler_spec make_spec(int sampler, const std::vector<float>* tables, int timesteps, int t_max, int speedup) {
    dsd_sampler_spec s;
    memset(&s, 0, sizeof(s));
    s.struct_size = (int32_t)sizeof(s);
    s.sampler = sampler;
    s.timesteps = timesteps;
    s.tables = tables ? tables->data() : NULL;
    s.t_max = t_max;
    s.speedup = speedup;
    s.time_scale_factor = 1000.0;
    return s;
}

// builds, walks every field the way dsd_sample's validation does, frees
static void expect_ok(const dsd_sampler_spec& s, const char* what) {
    dsd_program* p = NULL;
    const int rc = dsd_program_build(&s, &p);
    if (rc != DSD_OK || !p) {
        fprintf(stderr, "%s: expected a program, got %d: %s\n", what, rc, dsd_last_error(NULL));
        ++g_bad;
        return;
    }
    bool ok = p->n_bufs >= 1 && p->result_buf >= 0 && p->result_buf < p->n_bufs && p->n_evals >= 0 && (p->n_evals == 0 || p->evals);
    for (int i = 0; ok && i < p->n_evals; ++i) {
        const dsd_eval& e = p->evals[i];
        ok = e.x_buf >= 0 && e.x_buf < p->n_bufs && e.n_out >= 1 && e.n_out <= DSD_MAX_OUT && e.t == e.t;
        for (int o = 0; ok && o < e.n_out; ++o) {
            const dsd_lincomb& lc = e.out[o];
            ok = lc.dst >= 0 && lc.dst < p->n_bufs && lc.n_terms >= 1 && lc.n_terms <= DSD_MAX_TERMS;
            for (int k = 0; ok && k < lc.n_terms; ++k) {
                const int src = lc.terms[k].src;
                ok = ((src >= 0 && src < p->n_bufs) || src == DSD_SRC_MODEL ||
                      (src <= DSD_SRC_NOISE_BASE && DSD_SRC_NOISE_BASE - src < p->n_noise)) &&
                     isfinite(lc.terms[k].coef);
            }
        }
    }
    if (!ok) {
        fprintf(stderr, "%s: malformed program\n", what);
        ++g_bad;
    }
    dsd_program_free(p);
    ++g_built;
}

static void expect_einval(const dsd_sampler_spec* s, const char* what) {
    dsd_program* const sentinel = (dsd_program*)(uintptr_t)0x5a5a5a50;
    dsd_program* p = sentinel;
    const int rc = dsd_program_build(s, &p);
    if (rc != DSD_EINVAL || p != sentinel || !*dsd_last_error(NULL)) {
        fprintf(stderr, "%s: expected DSD_EINVAL with *out untouched, got %d\n", what, rc);
        ++g_bad;
        if (rc == DSD_OK && p != sentinel) dsd_program_free(p);
    }
    ++g_refused;
}

int main() {
    // tables: every case of the table tests, each into an allocation of exactly its size
    const int table_steps[] = {1000, 100, 4, 1};
    const double max_betas[] = {0.01, 0.02, 0.06};
    for (int t : table_steps)
        for (double mb : max_betas)
            for (int kind : {DSD_SCHEDULE_LINEAR, DSD_SCHEDULE_COSINE}) {
                std::vector<float> out((size_t)DSD_DDPM_TABLES * t);
                if (dsd_ddpm_tables_fill(kind, t, mb, out.data()) != DSD_OK) ++g_bad;
            }
    float one = 0.0f;
    if (dsd_ddpm_tables_fill(DSD_SCHEDULE_LINEAR, 4, 0.01, NULL) != DSD_EINVAL) ++g_bad;
    if (dsd_ddpm_tables_fill(2, 4, 0.01, &one) != DSD_EINVAL) ++g_bad;
    if (dsd_ddpm_tables_fill(DSD_SCHEDULE_LINEAR, 0, 0.01, &one) != DSD_EINVAL) ++g_bad;

    std::vector<float> tb((size_t)DSD_DDPM_TABLES * 1000), tb20((size_t)DSD_DDPM_TABLES * 20);
    if (dsd_ddpm_tables_fill(DSD_SCHEDULE_LINEAR, 1000, 0.01, tb.data()) != DSD_OK) return 1;
    if (dsd_ddpm_tables_fill(DSD_SCHEDULE_COSINE, 20, 0.0, tb20.data()) != DSD_OK) return 1;

    // the DDPM family over the grid (and a t_max that is no multiple of the speed-up, speed-up 1, the whole ancestral loop)
    const int grid[][2] = {{1000, 10}, {1000, 100}, {200, 10}, {400, 20}, {20, 20}, {1000, 7}, {1000, 1000}, {999, 10},
                           {1000, 1}, {1000, 50}, {1000, 20}, {1000, 200}, {20, 10}, {0, 10}, {1, 1}};
    for (const auto& g : grid)
        for (int sampler = DSD_SAMPLER_DDPM; sampler <= DSD_SAMPLER_UNIPC; ++sampler) {
            const bool solver = sampler == DSD_SAMPLER_DPM_SOLVER_PP || sampler == DSD_SAMPLER_UNIPC;
            if (solver && g[0] != 0 && g[0] / g[1] < 2) continue;       // refused below
            expect_ok(make_spec(sampler, &tb, 1000, g[0], g[1]), "grid");
        }
    // tables exactly as long as t_max: the last entry read is the last one there
    for (int sampler = DSD_SAMPLER_DDPM; sampler <= DSD_SAMPLER_UNIPC; ++sampler) {
        expect_ok(make_spec(sampler, &tb20, 20, 20, 1), "20 of 20");
        expect_ok(make_spec(sampler, &tb20, 20, 20, 10), "20 of 20 by 10");
    }
    // ancestral chunks
    for (const auto& c : {std::vector<int>{20, 8, 0}, {8, 0, 12}, {1000, 950, 0}, {1000, 0, 7}, {5, 5, 3}}) {
        dsd_sampler_spec s = make_spec(DSD_SAMPLER_DDPM, &tb, 1000, c[0], 1);
        s.t_lo = c[1];
        s.noise_index0 = c[2];
        expect_ok(s, "ancestral chunk");
    }
    // rectified flow
    for (int sampler = DSD_SAMPLER_RF_EULER; sampler <= DSD_SAMPLER_RF_EULER_ONNX; ++sampler)
        for (int steps : {0, 1, 3, 7, 20, 1000})
            for (double t_start : {0.0, 0.4, 0.123456789, 1.0}) {
                dsd_sampler_spec s = make_spec(sampler, NULL, 0, 0, 0);
                s.steps = steps;
                s.t_start = t_start;
                expect_ok(s, "reflow");
            }

    // every refused case
    expect_einval(NULL, "null spec");
    {
        dsd_sampler_spec s = make_spec(DSD_SAMPLER_DDIM, &tb, 1000, 1000, 10);
        if (dsd_program_build(&s, NULL) != DSD_EINVAL) ++g_bad;
        s.struct_size = 48;
        expect_einval(&s, "short struct");
        s.struct_size = 0;
        expect_einval(&s, "zero struct");
    }
    for (int sampler : {-1, 10, 1 << 30}) {
        const dsd_sampler_spec s = make_spec(sampler, &tb, 1000, 1000, 10);
        expect_einval(&s, "unknown sampler");
    }
    for (int sampler : {DSD_SAMPLER_DPM_SOLVER_PP, DSD_SAMPLER_UNIPC})
        for (const auto& g : {std::vector<int>{1000, 1000}, {1000, 501}, {10, 20}, {1, 1}}) {
            const dsd_sampler_spec s = make_spec(sampler, &tb, 1000, g[0], g[1]);
            expect_einval(&s, "fewer than 2 steps");
        }
    for (int sampler = DSD_SAMPLER_DDPM; sampler <= DSD_SAMPLER_UNIPC; ++sampler) {
        dsd_sampler_spec s = make_spec(sampler, &tb, 1000, 1001, 10);
        expect_einval(&s, "t_max > timesteps");
        s = make_spec(sampler, &tb, 1000, -1, 10);
        expect_einval(&s, "t_max < 0");
        s = make_spec(sampler, &tb, 1000, 1000, 0);
        expect_einval(&s, "speedup 0");
        s = make_spec(sampler, &tb, 1000, 1000, -3);
        expect_einval(&s, "speedup < 0");
        s = make_spec(sampler, NULL, 1000, 1000, 10);
        expect_einval(&s, "null tables");
        s = make_spec(sampler, &tb, 0, 0, 10);
        expect_einval(&s, "timesteps 0");
    }
    {
        dsd_sampler_spec s = make_spec(DSD_SAMPLER_DDPM, &tb, 1000, 20, 1);
        s.t_lo = 21;
        expect_einval(&s, "t_lo > t_max");
        s.t_lo = -1;
        expect_einval(&s, "t_lo < 0");
        s.t_lo = 0;
        s.noise_index0 = -1;
        expect_einval(&s, "noise_index0 < 0");
        s.noise_index0 = INT32_MAX;
        expect_einval(&s, "noise_index0 overflow");
        s = make_spec(DSD_SAMPLER_RF_RK5, NULL, 0, 0, 0);
        s.steps = -1;
        expect_einval(&s, "reflow steps < 0");
        s.steps = 3;
        s.t_start = NAN;
        expect_einval(&s, "reflow NaN");
    }

    // the ONNX twins' plan
    std::vector<int64_t> factors;
    for (int i = 1; i <= 1000; ++i)
        if (1000 % i == 0) factors.push_back(i);
    int32_t t_max = 0, speedup = 0;
    for (int steps = 1; steps <= 1000; ++steps)
        for (int d = -1; d <= 100; ++d)
            if (dsd_onnx_ddpm_plan(1000, d % 2 ? 1000 : 400, factors.data(), (int32_t)factors.size(), steps, d < 0 ? -1.0 : 0.01 * d,
                                   &t_max, &speedup) != DSD_OK || speedup < 1 || t_max < 0 || t_max > 1000)
                ++g_bad;
    if (dsd_onnx_ddpm_plan(1000, 1000, factors.data(), (int32_t)factors.size(), 1, 1e30, &t_max, &speedup) != DSD_OK) ++g_bad;
    if (dsd_onnx_ddpm_plan(1000, 1000, NULL, 0, 10, -1.0, &t_max, &speedup) != DSD_EINVAL) ++g_bad;
    if (dsd_onnx_ddpm_plan(1000, 1000, factors.data(), (int32_t)factors.size(), 0, 0.5, &t_max, &speedup) != DSD_EINVAL) ++g_bad;
    if (dsd_onnx_ddpm_plan(1000, 1000, factors.data(), (int32_t)factors.size(), 10, 0.5, NULL, &speedup) != DSD_EINVAL) ++g_bad;
    if (dsd_onnx_ddpm_plan(1000, 1000, factors.data() + 1, 3, 1000, -1.0, &t_max, &speedup) != DSD_EINVAL) ++g_bad;
    dsd_program_free(NULL);

    printf("program_harness: %d programs built and freed, %d refused, %d unexpected results\n", g_built, g_refused, g_bad);
    return g_bad ? 1 : 0;
}
