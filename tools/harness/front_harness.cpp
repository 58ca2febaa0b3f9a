// Stand-alone memory check of the segment front end's host side (diffsinger_amd/csrc/curve_api.hip is host code only):
// dsd_seconds_to_frames over heap arrays of exactly n elements, and dsd_curve_resample's argument checks with the launcher
// replaced by plain loops over heap arrays of exactly n_points / pad_to elements, under the host compiler's address and
// undefined-behaviour sanitizers.  An argument set that the checks let through but that reaches outside the arrays is a heap
// overflow the sanitizer reports; a float -> integer conversion out of range in the frame arithmetic is undefined behaviour
// it reports too.  Not a test of the values (tests/test_front_host.py and tests/test_gpu_front.py hold them against torch,
// numpy and the reference's results): what this looks for is a read or write outside the arrays, an overflow, a frame or
// pad element nobody wrote.  Host only - never loaded into Python, needs no GPU:
//
// (one command line)
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude
//       tools/harness/front_harness.cpp -x c++ diffsinger_amd/csrc/curve_api.hip -o /tmp/front_harness
//   /tmp/front_harness              # prints the number of calls run and refused; exit status 0 = clean
//
// The library proper takes dsd::fail, dsd::select_device and dsd_last_error from api.hip; this program brings its own.
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <limits>
#include <string>
#include <vector>

#include "dsdenoise.h"
#include "../../diffsinger_amd/csrc/curve_params.h"

struct dsd_handle;
static std::string g_error;
static int g_launches = 0;
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
int select_device(const char*, int, bool) { return DSD_OK; }
// the indexing of curve_kernels.hip as loops (the finishing ops are arithmetic on the value and touch no memory)
const char* launch_curve_resample(const CurveBatch& b, void*) {
    ++g_launches;
    for (int i = 0; i < b.n; ++i) {
        const CurveD& c = b.c[i];
        for (int t = 0; t < c.pad_to; ++t) {
            if (t >= c.length) {
                c.out[t] = 0.f;
                if (c.uv) c.uv[t] = 0;
                continue;
            }
            const int k = t < c.valid - 1 ? t : c.valid - 1;
            const double x = (double)k * c.dst_step;
            const int last = c.n_points - 1;
            int j = (int)fmin(x / c.src_step, (double)last);
            while (j > 0 && c.src_step * (double)j > x) --j;
            while (j < last && c.src_step * (double)(j + 1) <= x) ++j;
            float v;
            if (j >= last) {
                v = c.points[last];
            } else {
                const double xj = c.src_step * (double)j, pj = (double)c.points[j];
                v = xj == x ? (float)pj : (float)((((double)c.points[j + 1] - pj) / (c.src_step * (double)(j + 1) - xj)) * (x - xj) + pj);
            }
            c.out[t] = v;
            if (c.uv) c.uv[t] = v == 0.f;
        }
    }
    return nullptr;
}
}  // namespace dsd
extern "C" const char* dsd_last_error(const dsd_handle*) { return g_error.c_str(); }

static int g_ran = 0, g_refused = 0, g_bad = 0;

static void bad(const char* what) {
    fprintf(stderr, "%s (last error: %s)\n", what, g_error.c_str());
    ++g_bad;
}

static int g_launches_seen = 0;
// a refused call returns DSD_EINVAL, leaves a message and launches nothing
static void refused(int rc, const char* what) {
    if (rc != DSD_EINVAL || g_error.empty() || g_launches != g_launches_seen) bad(what);
    g_launches_seen = g_launches;
    g_error.clear();
    ++g_refused;
}

static unsigned g_seed = 2700;
static double uniform() {       // a small LCG: the values do not matter, the sizes do
    g_seed = g_seed * 1664525u + 1013904223u;
    return (double)(g_seed >> 8) / (double)(1u << 24);
}

// dsd_seconds_to_frames on exactly sized heap arrays: every output written, the total their sum, nothing negative
static void run_frames(int n, double timestep, double scale) {
    std::vector<float> sec((size_t)n);
    for (float& s : sec) s = (float)(uniform() * scale);
    if (n > 2) sec[(size_t)n / 2] = 0.f;
    std::vector<int64_t> frames((size_t)n, std::numeric_limits<int64_t>::min());
    int64_t total = -1, sum = 0;
    if (dsd_seconds_to_frames(sec.data(), n, timestep, frames.data(), &total) != DSD_OK) return bad("seconds_to_frames refused good input");
    for (int64_t f : frames) {
        if (f < 0) return bad("a frame count is negative or was never written");
        sum += f;
    }
    if (sum != total) bad("the total is not the sum of the frames");
    ++g_ran;
}

// dsd_curve_resample on exactly sized heap arrays through the stand-in launcher
static void run_curves(int n_curves) {
    std::vector<std::vector<float>> points((size_t)n_curves), outs((size_t)n_curves);
    std::vector<std::vector<uint8_t>> uvs((size_t)n_curves);
    std::vector<dsd_curve> cs((size_t)n_curves);
    const double steps[] = {0.005, 0.01, 0.02, 512.0 / 44100.0, 256.0 / 44100.0, 128.0 / 24000.0, 0.0116099773};
    for (int i = 0; i < n_curves; ++i) {
        dsd_curve& c = cs[(size_t)i];
        memset(&c, 0, sizeof(c));
        c.n_points = 2 + (int)(uniform() * 398.0);
        c.src_step = steps[(int)(uniform() * 7.0) % 7];
        c.dst_step = steps[(int)(uniform() * 7.0) % 7];
        const int count = (int)ceil(((double)(c.n_points - 1) * c.src_step) / c.dst_step);
        c.length = count - 5 + (int)(uniform() * 11.0);
        if (c.length < 1) c.length = 1;
        c.pad_to = c.length + (i % 3 == 0 ? 0 : (int)(uniform() * 300.0));
        c.op = i % 4;
        c.lo = c.op == DSD_CURVE_GENDER ? -5.f : 0.5f;
        c.hi = c.op == DSD_CURVE_GENDER ? 5.f : 2.f;
        points[(size_t)i].assign((size_t)c.n_points, 1.f);
        outs[(size_t)i].assign((size_t)c.pad_to, std::numeric_limits<float>::quiet_NaN());
        c.points = points[(size_t)i].data();
        c.out = outs[(size_t)i].data();
        if (c.op == DSD_CURVE_PITCH && i % 8 == 3) {
            uvs[(size_t)i].assign((size_t)c.pad_to, 0xff);
            c.uv_out = uvs[(size_t)i].data();
        }
    }
    if (dsd_curve_resample(0, cs.data(), n_curves, nullptr) != DSD_OK) return bad("curve_resample refused good input");
    for (int i = 0; i < n_curves; ++i) {
        for (float v : outs[(size_t)i])
            if (v != v) return bad("an output element was never written");
        for (uint8_t u : uvs[(size_t)i])
            if (u == 0xff) return bad("a uv element was never written");
    }
    ++g_ran;
}

int main() {
    const double steps[] = {0.005, 0.01, 512.0 / 44100.0, 0.0116099773};
    for (int n : {1, 2, 3, 17, 199, 2048})
        for (double step : steps) run_frames(n, step, 0.6);
    run_frames(5, 1e-3, 4.0e5);                     // boundaries up to 2e9 frames: they still fit
    for (int n : {1, 2, 7, 31, 32}) run_curves(n);
    g_launches_seen = g_launches;

    // dsd_seconds_to_frames: every refusal
    {
        const float ok[2] = {0.1f, 0.2f};
        int64_t frames[2], total;
        refused(dsd_seconds_to_frames(nullptr, 2, 0.01, frames, &total), "null seconds");
        refused(dsd_seconds_to_frames(ok, 2, 0.01, nullptr, &total), "null frames_out");
        refused(dsd_seconds_to_frames(ok, 2, 0.01, frames, nullptr), "null total_out");
        refused(dsd_seconds_to_frames(ok, 0, 0.01, frames, &total), "n 0");
        refused(dsd_seconds_to_frames(ok, -1, 0.01, frames, &total), "n < 0");
        refused(dsd_seconds_to_frames(ok, INT32_MIN, 0.01, frames, &total), "n INT32_MIN");
        for (double step : {0.0, -0.01, (double)NAN, (double)INFINITY, -(double)INFINITY, 1e-60, 1e60, 1e300})
            refused(dsd_seconds_to_frames(ok, 2, step, frames, &total), "bad timestep");
        for (float s : {NAN, INFINITY, -INFINITY, -1e-9f, -1.f}) {
            const float in[2] = {0.1f, s};
            refused(dsd_seconds_to_frames(in, 2, 0.01, frames, &total), "bad duration");
        }
        const float far[2] = {1.f, 3.0e7f}, huge[2] = {3.0e38f, 3.0e38f}, edge[1] = {2147483648.f};
        refused(dsd_seconds_to_frames(far, 2, 0.01, frames, &total), "3e9 frames");
        refused(dsd_seconds_to_frames(huge, 2, 1.0, frames, &total), "the prefix is inf");
        refused(dsd_seconds_to_frames(edge, 1, 1.0, frames, &total), "2^31 frames");
        refused(dsd_seconds_to_frames(huge, 2, 1e-30, frames, &total), "the quotient is inf");
        const float fits[1] = {2147483000.f};
        if (dsd_seconds_to_frames(fits, 1, 1.0, frames, &total) != DSD_OK || total != 2147483008) bad("the largest boundaries fit");
    }

    // dsd_curve_resample: every refusal, on a valid descriptor with one field changed
    {
        std::vector<float> pts(8, 1.f), out(6, 0.f);
        std::vector<uint8_t> uv(6, 0);
        dsd_curve good;
        memset(&good, 0, sizeof(good));
        good.points = pts.data(); good.out = out.data();
        good.src_step = 0.005; good.dst_step = 512.0 / 44100.0;
        good.n_points = 8; good.length = 4; good.pad_to = 6; good.op = DSD_CURVE_PLAIN;
        refused(dsd_curve_resample(0, nullptr, 1, nullptr), "null curves");
        refused(dsd_curve_resample(0, &good, 0, nullptr), "n_curves 0");
        refused(dsd_curve_resample(0, &good, -1, nullptr), "n_curves < 0");
        refused(dsd_curve_resample(0, &good, 33, nullptr), "n_curves 33");
        refused(dsd_curve_resample(0, &good, INT32_MAX, nullptr), "n_curves INT32_MAX");
        auto with = [&](auto change, const char* what) {
            dsd_curve two[2] = {good, good};
            change(two[1]);
            refused(dsd_curve_resample(0, two, 2, nullptr), what);
        };
        with([](dsd_curve& c) { c.points = nullptr; }, "null points");
        with([](dsd_curve& c) { c.out = nullptr; }, "null out");
        with([](dsd_curve& c) { c.n_points = 1; }, "n_points 1");
        with([](dsd_curve& c) { c.n_points = 0; }, "n_points 0");
        with([](dsd_curve& c) { c.n_points = INT32_MIN; }, "n_points INT32_MIN");
        with([](dsd_curve& c) { c.length = 0; }, "length 0");
        with([](dsd_curve& c) { c.length = -4; }, "length < 0");
        with([](dsd_curve& c) { c.pad_to = 3; }, "pad_to below length");
        with([](dsd_curve& c) { c.pad_to = INT32_MIN; }, "pad_to INT32_MIN");
        with([](dsd_curve& c) { c.src_step = 0.0; }, "src_step 0");
        with([](dsd_curve& c) { c.src_step = -0.005; }, "src_step < 0");
        with([](dsd_curve& c) { c.src_step = NAN; }, "src_step NaN");
        with([](dsd_curve& c) { c.src_step = INFINITY; }, "src_step inf");
        with([](dsd_curve& c) { c.dst_step = 0.0; }, "dst_step 0");
        with([](dsd_curve& c) { c.dst_step = -1.0; }, "dst_step < 0");
        with([](dsd_curve& c) { c.dst_step = NAN; }, "dst_step NaN");
        with([](dsd_curve& c) { c.dst_step = INFINITY; }, "dst_step inf");
        with([](dsd_curve& c) { c.src_step = 1e-300; c.dst_step = 1e300; }, "no frame");
        with([](dsd_curve& c) { c.op = 4; }, "op 4");
        with([](dsd_curve& c) { c.op = -1; }, "op -1");
        with([](dsd_curve& c) { c.op = DSD_CURVE_CLIP; c.lo = 1.f; c.hi = 0.5f; }, "CLIP lo > hi");
        with([](dsd_curve& c) { c.op = DSD_CURVE_CLIP; c.lo = NAN; c.hi = 0.5f; }, "CLIP NaN lo");
        with([](dsd_curve& c) { c.op = DSD_CURVE_CLIP; c.lo = 0.f; c.hi = NAN; }, "CLIP NaN hi");
        with([](dsd_curve& c) { c.op = DSD_CURVE_GENDER; c.lo = 1.f; c.hi = 5.f; }, "GENDER lo > 0");
        with([](dsd_curve& c) { c.op = DSD_CURVE_GENDER; c.lo = -5.f; c.hi = -1.f; }, "GENDER hi < 0");
        with([](dsd_curve& c) { c.op = DSD_CURVE_GENDER; c.lo = -INFINITY; c.hi = 5.f; }, "GENDER inf");
        with([&](dsd_curve& c) { c.uv_out = uv.data(); }, "uv_out on PLAIN");
        // the edges that are allowed: a huge count against a short length, a tiny ratio that still leaves one frame
        dsd_curve edge = good;
        edge.src_step = 1e6; edge.dst_step = 1e-6; edge.length = 6;
        if (dsd_curve_resample(0, &edge, 1, nullptr) != DSD_OK) bad("a count past int32 is cut to the length");
        edge = good;
        edge.src_step = 1e-6; edge.dst_step = 1e3;
        if (dsd_curve_resample(0, &edge, 1, nullptr) != DSD_OK) bad("one frame");
        edge = good;
        edge.op = DSD_CURVE_PITCH; edge.uv_out = uv.data();
        if (dsd_curve_resample(0, &edge, 1, nullptr) != DSD_OK) bad("uv_out on PITCH");
        g_launches_seen = g_launches;
    }

    printf("front_harness: %d calls run on exactly sized arrays, %d calls refused, %d unexpected results\n", g_ran, g_refused, g_bad);
    return g_bad ? 1 : 0;
}
