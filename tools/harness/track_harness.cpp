// Stand-alone memory check of the track entries' host side (diffsinger_amd/csrc/track_api.hip is host code only):
// dsd_track_plan and the argument checks of dsd_track_place / _peak / _export on every G24 layout (the layouts of
// tests/track_ref.py, restated below as data) and on every refusal, under the host compiler's address and
// undefined-behaviour sanitizers.  The library proper launches kernels behind the checks; here the three launchers are
// plain loops over heap arrays of exactly `total` elements, so an argument set that the checks let through but that
// reaches outside the track is a heap overflow the sanitizer reports.  Not a test of the values (the pytest files hold
// them against the oracle): what this looks for is a read or write outside the arrays, an integer overflow in the
// geometry, a sample no placement wrote.  Host only - never loaded into Python, needs no GPU:
//
// (one command line)
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude
//       tools/harness/track_harness.cpp -x c++ diffsinger_amd/csrc/track_api.hip -o /tmp/track_harness
//   /tmp/track_harness              # prints the number of layouts placed and calls refused; exit status 0 = clean
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
// the rule of include/dsdenoise.h as loops
const char* launch_track_place(double* track, long long s, long long p, const float* src, long long n, void*) {
    ++g_launches;
    const long long F = p - s;
    for (long long i = p; i < s; ++i) track[i] = 0.0;
    for (long long j = 0; j < n; ++j) {
        if (j < F) {
            const double r = F == 1 ? 0.0 : j == F - 1 ? 1.0 : (double)j * (1.0 / (double)(F - 1));
            track[s + j] = (1.0 - r) * track[s + j] + r * (double)src[j];
        } else {
            track[s + j] = (double)src[j];
        }
    }
    return nullptr;
}
const char* launch_track_peak(const double* track, long long total, double* peak_out, void*) {
    ++g_launches;
    double m = 0.0;
    for (long long i = 0; i < total; ++i) m = fabs(track[i]) > m ? fabs(track[i]) : m;
    *peak_out = m;
    return nullptr;
}
const char* launch_track_export(const double* track, long long total, int kind, const double* peak, void* out, void*) {
    ++g_launches;
    for (long long i = 0; i < total; ++i) {
        if (kind == DSD_TRACK_F64) static_cast<double*>(out)[i] = track[i];
        else if (kind == DSD_TRACK_F32) static_cast<float*>(out)[i] = (float)track[i];
        else {
            double x = peak ? (*peak == 0.0 ? 0.0 : track[i] / *peak * 32767.0) : track[i] * 32767.0;
            x = x != x ? 0.0 : x < -32768.0 ? -32768.0 : x > 32767.0 ? 32767.0 : x;
            static_cast<int16_t*>(out)[i] = (int16_t)x;
        }
    }
    return nullptr;
}
}  // namespace dsd
extern "C" const char* dsd_last_error(const dsd_handle*) { return g_error.c_str(); }

static int g_placed = 0, g_refused = 0, g_bad = 0;

static void bad(const char* what) {
    fprintf(stderr, "%s (last error: %s)\n", what, g_error.c_str());
    ++g_bad;
}

struct Layout {
    const char* name;
    int sample_rate;
    std::vector<double> offsets;
    std::vector<int64_t> lengths;
};

// tests/track_ref.py: LAYOUTS ...
static const Layout kLayouts[] = {
    {"overlap_gap", 44100, {0 / 44100.0, 353 / 44100.0, 882 / 44100.0}, {400, 300, 350}},
    {"silence_first", 44100, {127 / 44100.0, 427 / 44100.0, 528 / 44100.0}, {300, 100, 77}},
    {"inside_fade", 44100, {0 / 44100.0, 300 / 44100.0, 350 / 44100.0}, {400, 200, 300}},
    {"before_predecessor", 44100, {0 / 44100.0, 250 / 44100.0, 200 / 44100.0}, {300, 60, 200}},
    {"fade_one_two", 44100, {0 / 44100.0, 199 / 44100.0, 247 / 44100.0}, {200, 50, 30}},
    {"fade_whole", 44100, {3 / 44100.0, 253 / 44100.0, 303 / 44100.0}, {300, 50, 41}},
    {"halves", 16000, {2.5 / 16000, 0.0125 + 3.5 / 16000, 0.02}, {150, 100, 1}},
    {"single", 16000, {0.001}, {333}},
};
// ... and MALFORMED
static const Layout kMalformed[] = {
    {"negative_first", 44100, {-3 / 44100.0}, {10}},
    {"fade_too_long", 44100, {0 / 44100.0, 50 / 44100.0}, {100, 20}},
    {"negative_later", 44100, {0.0, 40 / 44100.0, -2 / 44100.0}, {50, 30, 200}},
};

// plan, place every segment into an exactly sized heap track, peak, the three exports
static void run_layout(const Layout& L) {
    const int n = (int)L.offsets.size();
    std::vector<int64_t> starts(n), ends(n);
    int64_t total = -1;
    if (dsd_track_plan(n, L.offsets.data(), L.lengths.data(), L.sample_rate, starts.data(), ends.data(), &total) != DSD_OK || total < 1)
        return bad(L.name);
    std::vector<double> track((size_t)total, std::numeric_limits<double>::quiet_NaN());
    for (int k = 0; k < n; ++k) {
        std::vector<float> seg((size_t)L.lengths[k]);
        for (size_t i = 0; i < seg.size(); ++i) seg[i] = (float)((int)((i * 37 + k * 11) % 201) - 100) / 128.0f;
        if (dsd_track_place(0, track.data(), total, starts[k], ends[k], seg.data(), L.lengths[k], nullptr) != DSD_OK) return bad(L.name);
    }
    for (double v : track)
        if (v != v) return bad("a sample was never written");
    double peak = -1.0;
    std::vector<double> f64((size_t)total);
    std::vector<float> f32((size_t)total);
    std::vector<int16_t> pcm((size_t)total);
    if (dsd_track_peak(0, track.data(), total, &peak, nullptr) != DSD_OK || !(peak > 0.0)) return bad(L.name);
    if (dsd_track_export(0, track.data(), total, DSD_TRACK_F64, nullptr, f64.data(), nullptr) != DSD_OK) return bad(L.name);
    if (dsd_track_export(0, track.data(), total, DSD_TRACK_F32, nullptr, f32.data(), nullptr) != DSD_OK) return bad(L.name);
    if (dsd_track_export(0, track.data(), total, DSD_TRACK_PCM, nullptr, pcm.data(), nullptr) != DSD_OK) return bad(L.name);
    if (dsd_track_export(0, track.data(), total, DSD_TRACK_PCM, &peak, pcm.data(), nullptr) != DSD_OK) return bad(L.name);
    ++g_placed;
}

// a refused call returns DSD_EINVAL, leaves a message and launches nothing
static int g_launches_seen = 0;        // main() brings it up to date after the calls that are meant to launch
static void refused(int rc, const char* what) {
    if (rc != DSD_EINVAL || g_error.empty() || g_launches != g_launches_seen) bad(what);
    g_launches_seen = g_launches;
    g_error.clear();
    ++g_refused;
}

int main() {
    for (const Layout& L : kLayouts) run_layout(L);
    g_launches_seen = g_launches;

    // dsd_track_plan: every refusal
    for (const Layout& L : kMalformed) {
        std::vector<int64_t> s(L.offsets.size()), e(L.offsets.size());
        int64_t total = 0;
        refused(dsd_track_plan((int)L.offsets.size(), L.offsets.data(), L.lengths.data(), L.sample_rate, s.data(), e.data(), &total), L.name);
    }
    {
        const double off[2] = {0.0, 1.0};
        const int64_t len[2] = {5, 5};
        int64_t s[2], e[2], total;
        refused(dsd_track_plan(2, nullptr, len, 10, s, e, &total), "null offsets");
        refused(dsd_track_plan(2, off, nullptr, 10, s, e, &total), "null lengths");
        refused(dsd_track_plan(2, off, len, 10, nullptr, e, &total), "null starts");
        refused(dsd_track_plan(2, off, len, 10, s, nullptr, &total), "null prev_ends");
        refused(dsd_track_plan(2, off, len, 10, s, e, nullptr), "null total");
        refused(dsd_track_plan(0, off, len, 10, s, e, &total), "n_seg 0");
        refused(dsd_track_plan(-2, off, len, 10, s, e, &total), "n_seg < 0");
        refused(dsd_track_plan(2, off, len, 0, s, e, &total), "sample_rate 0");
        refused(dsd_track_plan(2, off, len, -1, s, e, &total), "sample_rate < 0");
        const int64_t zero_len[2] = {5, 0}, neg_len[2] = {-1, 5}, huge_len[2] = {5, INT64_MAX}, big_len[2] = {5, (int64_t)1 << 31};
        refused(dsd_track_plan(2, off, zero_len, 10, s, e, &total), "length 0");
        refused(dsd_track_plan(2, off, neg_len, 10, s, e, &total), "length < 0");
        refused(dsd_track_plan(2, off, huge_len, 10, s, e, &total), "length INT64_MAX");
        refused(dsd_track_plan(2, off, big_len, 10, s, e, &total), "length 2^31");
        const double nan_off[2] = {0.0, NAN}, inf_off[2] = {0.0, INFINITY}, ninf_off[2] = {0.0, -INFINITY}, far_off[2] = {0.0, 1e300},
                     edge_off[2] = {0.0, 2147483643.0};
        refused(dsd_track_plan(2, nan_off, len, 10, s, e, &total), "NaN offset");
        refused(dsd_track_plan(2, inf_off, len, 10, s, e, &total), "inf offset");
        refused(dsd_track_plan(2, ninf_off, len, 10, s, e, &total), "-inf offset");
        refused(dsd_track_plan(2, far_off, len, 10, s, e, &total), "offset 1e300");
        refused(dsd_track_plan(2, edge_off, len, 1, s, e, &total), "total 2^31");
        const int64_t fit_len[2] = {5, 4};
        if (dsd_track_plan(2, edge_off, fit_len, 1, s, e, &total) != DSD_OK || total != INT32_MAX) bad("total 2^31 - 1 is allowed");
    }

    // dsd_track_place: every refusal of its own geometry, on a 100-sample heap track and a 20-sample segment
    {
        std::vector<double> track(100, 0.0);
        std::vector<float> seg(20, 0.5f);
        double* t = track.data();
        const float* s = seg.data();
        refused(dsd_track_place(0, nullptr, 100, 10, 5, s, 20, nullptr), "null track");
        refused(dsd_track_place(0, t, 100, 10, 5, nullptr, 20, nullptr), "null src");
        refused(dsd_track_place(0, t, 0, 10, 5, s, 20, nullptr), "total 0");
        refused(dsd_track_place(0, t, (int64_t)1 << 31, 10, 5, s, 20, nullptr), "total 2^31");
        refused(dsd_track_place(0, t, 100, 10, 5, s, 0, nullptr), "n 0");
        refused(dsd_track_place(0, t, 100, 10, 5, s, -20, nullptr), "n < 0");
        refused(dsd_track_place(0, t, 100, -1, 5, s, 20, nullptr), "start < 0");
        refused(dsd_track_place(0, t, 100, INT64_MIN, 5, s, 20, nullptr), "start INT64_MIN");
        refused(dsd_track_place(0, t, 100, 81, 5, s, 20, nullptr), "end past the track");
        refused(dsd_track_place(0, t, 100, 101, 5, s, 1, nullptr), "start past the track");
        refused(dsd_track_place(0, t, 100, INT64_MAX, 5, s, INT64_MAX, nullptr), "start + n overflows");
        refused(dsd_track_place(0, t, 100, 10, 5, s, INT64_MAX, nullptr), "n INT64_MAX");
        refused(dsd_track_place(0, t, 100, 10, -1, s, 20, nullptr), "prev_end < 0");
        refused(dsd_track_place(0, t, 100, 10, INT64_MIN, s, 20, nullptr), "prev_end INT64_MIN");
        refused(dsd_track_place(0, t, 100, 10, 101, s, 20, nullptr), "prev_end past the track");
        refused(dsd_track_place(0, t, 100, 10, INT64_MAX, s, 20, nullptr), "prev_end INT64_MAX");
        refused(dsd_track_place(0, t, 100, 10, 31, s, 20, nullptr), "fade longer than the segment");
        refused(dsd_track_place(0, (double*)((char*)t + 4), 100, 10, 5, s, 20, nullptr), "misaligned track");
        refused(dsd_track_place(0, t, 100, 10, 5, (const float*)((const char*)s + 2), 20, nullptr), "misaligned src");
        // the edges that are allowed: the whole track, the last sample, F == n, a gap up to the end
        if (dsd_track_place(0, t, 100, 80, 100, s, 20, nullptr) != DSD_OK) bad("F == n at the end");
        if (dsd_track_place(0, t, 100, 99, 0, s, 1, nullptr) != DSD_OK) bad("the last sample after a gap");
        std::vector<float> whole(100, 0.25f);
        if (dsd_track_place(0, t, 100, 0, 0, whole.data(), 100, nullptr) != DSD_OK) bad("the whole track");
        g_launches_seen = g_launches;
    }

    // dsd_track_peak / dsd_track_export: every refusal
    {
        std::vector<double> track(10, 0.5);
        std::vector<double> out(10);
        double peak = 0.0;
        const double* t = track.data();
        refused(dsd_track_peak(0, nullptr, 10, &peak, nullptr), "peak: null track");
        refused(dsd_track_peak(0, t, 10, nullptr, nullptr), "peak: null out");
        refused(dsd_track_peak(0, t, 0, &peak, nullptr), "peak: total 0");
        refused(dsd_track_peak(0, t, -5, &peak, nullptr), "peak: total < 0");
        refused(dsd_track_peak(0, t, (int64_t)1 << 31, &peak, nullptr), "peak: total 2^31");
        refused(dsd_track_peak(0, (const double*)((const char*)t + 1), 10, &peak, nullptr), "peak: misaligned track");
        refused(dsd_track_peak(0, t, 10, (double*)((char*)out.data() + 4), nullptr), "peak: misaligned out");
        refused(dsd_track_export(0, nullptr, 10, DSD_TRACK_PCM, nullptr, out.data(), nullptr), "export: null track");
        refused(dsd_track_export(0, t, 10, DSD_TRACK_PCM, nullptr, nullptr, nullptr), "export: null out");
        refused(dsd_track_export(0, t, 10, 3, nullptr, out.data(), nullptr), "export: kind 3");
        refused(dsd_track_export(0, t, 10, -1, nullptr, out.data(), nullptr), "export: kind -1");
        refused(dsd_track_export(0, t, 10, DSD_TRACK_F64, &peak, out.data(), nullptr), "export: peak with f64");
        refused(dsd_track_export(0, t, 10, DSD_TRACK_F32, &peak, out.data(), nullptr), "export: peak with f32");
        refused(dsd_track_export(0, t, 0, DSD_TRACK_PCM, nullptr, out.data(), nullptr), "export: total 0");
        refused(dsd_track_export(0, t, (int64_t)1 << 31, DSD_TRACK_PCM, nullptr, out.data(), nullptr), "export: total 2^31");
        refused(dsd_track_export(0, (const double*)((const char*)t + 4), 10, DSD_TRACK_PCM, nullptr, out.data(), nullptr), "export: misaligned track");
        refused(dsd_track_export(0, t, 10, DSD_TRACK_F64, nullptr, (char*)out.data() + 4, nullptr), "export: misaligned f64 out");
        refused(dsd_track_export(0, t, 10, DSD_TRACK_F32, nullptr, (char*)out.data() + 2, nullptr), "export: misaligned f32 out");
        refused(dsd_track_export(0, t, 10, DSD_TRACK_PCM, nullptr, (char*)out.data() + 1, nullptr), "export: misaligned pcm out");
        refused(dsd_track_export(0, t, 10, DSD_TRACK_PCM, (const double*)((const char*)&peak + 4), out.data(), nullptr), "export: misaligned peak");
    }

    printf("track_harness: %d layouts placed and exported, %d calls refused, %d unexpected results\n", g_placed, g_refused, g_bad);
    return g_bad ? 1 : 0;
}
