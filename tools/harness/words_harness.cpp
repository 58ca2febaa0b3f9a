// Stand-alone memory check of the score algebra's host side (diffsinger_amd/csrc/words_api.hip is host code only):
// the argument checks of dsd_word_dur, dsd_group_midi and dsd_rhythm_align, with the launchers replaced by plain loops that
// restate the kernels' indexing and arithmetic over heap arrays of exactly B * N / B * W / B * L elements, under the host
// compiler's address and undefined-behaviour sanitizers.  An argument set that the checks let through but that reaches
// outside the arrays is a heap overflow the sanitizer reports; an index used without its range check is one too.  Not a
// test of the values (tests/test_words_host.py and tests/test_gpu_words.py hold them against the reference's results): what
// this looks for is a read or write outside the arrays, an overflow, an output element nobody wrote.  Host only - never
// loaded into Python, needs no GPU:
//
// (one command line)
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude
//       tools/harness/words_harness.cpp -x c++ diffsinger_amd/csrc/words_api.hip -o /tmp/words_harness
//   /tmp/words_harness              # prints the number of calls run and refused; exit status 0 = clean
//
// The library proper takes dsd::fail, dsd::select_device and dsd_last_error from api.hip; this program brings its own.
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <limits>
#include <string>
#include <vector>

#include "dsdenoise.h"
#include "../../diffsinger_amd/csrc/words_params.h"

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

// sums[i] = min(v(0) + .. + v(i), cap) with every v cut to [0, cap]: what block_prefix_capped leaves in LDS
static std::vector<int> capped_sums(const int64_t* v, int n, int cap) {
    std::vector<int> c((size_t)n);
    int64_t run = 0;
    for (int i = 0; i < n; ++i) {
        run = std::min<int64_t>(run + (v[i] > 0 ? std::min<int64_t>(v[i], cap) : 0), cap);
        c[(size_t)i] = (int)run;
    }
    return c;
}

const char* launch_word_dur(const WordDurP& p, int items, void*) {
    ++g_launches;
    for (int k = 0; k < items; ++k) {
        const long b = p.b0 + k;
        std::vector<int64_t> wd((size_t)p.W, 0);
        int64_t count = 0;
        for (int i = 0; i < p.N; ++i) {
            if (p.slur) count += p.slur[b * p.N + i] ? 0 : 1;
            const int64_t idx = p.slur ? count : p.index[b * p.N + i];
            if (p.index_out) p.index_out[b * p.N + i] = idx;
            if (idx >= 1 && idx <= p.W) wd[(size_t)(idx - 1)] += p.dur[b * p.N + i];
        }
        int64_t* out = p.word_dur + b * p.W;
        if (!p.has_totals) {
            for (int w = 0; w < p.W; ++w) out[w] = wd[(size_t)w];
            continue;
        }
        const int total = p.total[k];
        const std::vector<int> c = capped_sums(wd.data(), p.W, total);
        int last = -1;
        for (int w = 0; w < p.W; ++w)
            if (wd[(size_t)w] > 0) last = w;
        for (int w = 0; w < p.W; ++w)
            out[w] = c[(size_t)w] - (w ? c[(size_t)w - 1] : 0) + (w == last ? total - c[(size_t)p.W - 1] : 0);
    }
    return nullptr;
}

const char* launch_group_midi(const GroupMidiP& p, int items, void*) {
    ++g_launches;
    for (long b = 0; b < items; ++b) {
        const std::vector<int> cn = capped_sums(p.note_dur + b * p.Nn, p.Nn, p.T), cg = capped_sums(p.group_dur + b * p.G, p.G, p.T);
        std::vector<float> r((size_t)p.G);
        for (int g = 0; g < p.G; ++g) {
            const int end = cg[(size_t)g];
            int f = g ? cg[(size_t)g - 1] : 0;
            float sum = 0.0f;
            if (f < end) {
                const float n = (float)p.group_dur[b * p.G + g];
                int j = (int)(std::upper_bound(cn.begin(), cn.end(), f) - cn.begin());
                while (f < end && j < p.Nn) {
                    const int stop = std::min(end, cn[(size_t)j]);
                    const float q = p.note_midi[b * p.Nn + j] / n;
                    for (; f < stop; ++f) sum = sum + q;
                    ++j;
                }
            }
            r[(size_t)g] = rintf(sum);
        }
        if (p.ph2word) {
            for (int i = 0; i < p.L; ++i) {
                const int64_t w = p.ph2word[b * p.L + i];
                p.midi[b * p.L + i] = (w >= 1 && w <= p.G) ? (int64_t)r[(size_t)(w - 1)] : 0;
            }
        } else {
            for (int g = 0; g < p.G; ++g) p.midi[b * p.G + g] = (int64_t)r[(size_t)g];
        }
    }
    return nullptr;
}

const char* launch_rhythm_align(const RhythmP& p, int items, void*) {
    ++g_launches;
    for (long b = 0; b < items; ++b) {
        std::vector<int> idx((size_t)p.L);
        std::vector<float> d((size_t)p.L), alpha((size_t)p.W);
        for (int i = 0; i < p.L; ++i) {
            const int64_t w = p.ph2word[b * p.L + i];
            idx[(size_t)i] = (w >= 1 && w <= p.W) ? (int)w : 0;
            d[(size_t)i] = p.pred[b * p.L + i] * (w > 0 ? 1.0f : 0.0f);
        }
        for (int w = 0; w < p.W; ++w) {
            float s = 0.0f;
            for (int i = 0; i < p.L; ++i)
                if (idx[(size_t)i] == w + 1) s = s + d[(size_t)i];
            alpha[(size_t)w] = (float)p.word_dur[b * p.W + w] / (s < 1e-5f ? 1e-5f : s);
        }
        for (int i = 0; i < p.L; ++i)
            p.out[b * p.L + i] = idx[(size_t)i] ? (int64_t)rintf(d[(size_t)i] * alpha[(size_t)idx[(size_t)i] - 1]) : 0;
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

static unsigned g_seed = 3000;
static int below(int n) {       // a small LCG: the values do not matter much, the sizes and the indices do
    g_seed = g_seed * 1664525u + 1013904223u;
    return (int)((g_seed >> 8) % (unsigned)n);
}

constexpr int64_t kUnset = std::numeric_limits<int64_t>::min();

static void run_word_dur(int B, int N, int W, bool slur, bool totals) {
    std::vector<int64_t> dur((size_t)B * N), index((size_t)B * N), wd((size_t)B * W, kUnset), idx_out((size_t)B * N, kUnset), tot((size_t)B);
    std::vector<uint8_t> sl((size_t)B * N);
    for (size_t i = 0; i < dur.size(); ++i) {
        dur[i] = below(40);
        index[i] = below(W + 4) - 2;        // some outside [1, W], on both sides
        sl[i] = below(3) == 0;
    }
    int64_t sum0 = 0;
    for (int i = 0; i < N; ++i) sum0 += dur[(size_t)i];
    for (int b = 0; b < B; ++b) tot[(size_t)b] = b % 3 == 0 ? sum0 : b % 3 == 1 ? below(20 * N + 1) : 40 * (int64_t)N + 7;
    dsd_word_dur_args a;
    memset(&a, 0, sizeof(a));
    a.struct_size = sizeof(a); a.B = B; a.N = N; a.W = W;
    a.dur = dur.data(); a.word_dur = wd.data(); a.index_out = idx_out.data();
    if (slur) a.slur = sl.data();
    else a.index = index.data();
    if (totals) a.totals = tot.data();
    if (dsd_word_dur(0, &a, nullptr) != DSD_OK) return bad("word_dur refused good input");
    for (int b = 0; b < B; ++b) {
        int64_t sum = 0, raw = 0;
        for (int w = 0; w < W; ++w) {
            const int64_t v = wd[(size_t)b * W + w];
            if (v < 0) return bad("a word duration is negative or was never written");
            sum += v;
        }
        for (int i = 0; i < N; ++i) {
            const int64_t ix = idx_out[(size_t)b * N + i];
            if (ix == kUnset) return bad("an index element was never written");
            if (ix >= 1 && ix <= W) raw += dur[(size_t)b * N + i];
        }
        if (totals ? (raw > 0 && sum != tot[(size_t)b]) || (raw == 0 && sum != 0) : sum != raw) return bad("the words do not sum to the total");
    }
    ++g_ran;
}

static void run_group_midi(int B, int Nn, int G, int L, int T) {
    std::vector<float> midi((size_t)B * Nn);
    std::vector<int64_t> nd((size_t)B * Nn), gd((size_t)B * G), p2w((size_t)B * std::max(L, 1)), out((size_t)B * (L ? L : G), kUnset);
    for (float& m : midi) m = 36.f + 0.25f * (float)below(200);
    for (int64_t& d : nd) d = below(2 * T / Nn + 3);
    for (int64_t& d : gd) d = below(3) ? below(2 * T / G + 3) : 0;
    for (int64_t& w : p2w) w = below(G + 4) - 2;
    dsd_group_midi_args a;
    memset(&a, 0, sizeof(a));
    a.struct_size = sizeof(a); a.B = B; a.Nn = Nn; a.G = G; a.L = L; a.T = T;
    a.note_midi = midi.data(); a.note_dur = nd.data(); a.group_dur = gd.data(); a.ph2word = L ? p2w.data() : nullptr; a.midi = out.data();
    if (dsd_group_midi(0, &a, nullptr) != DSD_OK) return bad("group_midi refused good input");
    for (int64_t v : out)
        if (v < 0 || v > 86) return bad("a MIDI value is outside the notes' range or was never written");
    ++g_ran;
}

static void run_rhythm(int B, int L, int W) {
    std::vector<float> pred((size_t)B * L);
    std::vector<int64_t> p2w((size_t)B * L), wd((size_t)B * W), out((size_t)B * L, kUnset);
    for (float& v : pred) v = 0.5f * (float)below(60);
    for (int64_t& w : p2w) w = below(W + 4) - 2;
    for (int64_t& d : wd) d = below(50);
    dsd_rhythm_align_args a;
    memset(&a, 0, sizeof(a));
    a.struct_size = sizeof(a); a.B = B; a.L = L; a.W = W;
    a.ph_dur_pred = pred.data(); a.ph2word = p2w.data(); a.word_dur = wd.data(); a.ph_dur = out.data();
    if (dsd_rhythm_align(0, &a, nullptr) != DSD_OK) return bad("rhythm_align refused good input");
    for (int64_t v : out)
        if (v < 0) return bad("a duration is negative or was never written");
    ++g_ran;
}

int main() {
    for (int B : {1, 3, 64, 65, 130})
        for (int N : {1, 7, 2048})
            for (int W : {1, 5, 2048}) {
                if ((long)B * N * W > 3l * 2048 * 2048) continue;
                for (int mode = 0; mode < 4; ++mode) run_word_dur(B, N, W, mode & 1, mode & 2);
            }
    for (int B : {1, 3})
        for (int Nn : {1, 9, 2048})
            for (int G : {1, 6, 2048})
                for (int L : {0, 1, 13, 2048}) run_group_midi(B, Nn, G, L, Nn == 2048 ? 4096 : 57);
    for (int B : {1, 3})
        for (int L : {1, 17, 2048})
            for (int W : {1, 7, 2048}) run_rhythm(B, L, W);
    g_launches_seen = g_launches;

    std::vector<int64_t> i64(64, 1);
    std::vector<uint8_t> u8(64, 0);
    std::vector<float> f32(64, 1.f);
    // dsd_word_dur: every refusal, on a valid struct with one field changed
    {
        int64_t tot[2] = {5, 6};
        dsd_word_dur_args good;
        memset(&good, 0, sizeof(good));
        good.struct_size = sizeof(good); good.B = 2; good.N = 8; good.W = 4;
        good.dur = i64.data(); good.index = i64.data(); good.word_dur = i64.data() + 32; good.totals = tot;
        refused(dsd_word_dur(0, nullptr, nullptr), "null args");
        auto with = [&](auto change, const char* what) {
            dsd_word_dur_args a = good;
            change(a);
            refused(dsd_word_dur(0, &a, nullptr), what);
        };
        with([](dsd_word_dur_args& a) { a.struct_size = 0; }, "struct_size 0");
        with([](dsd_word_dur_args& a) { a.struct_size -= 8; }, "struct_size short");
        with([](dsd_word_dur_args& a) { a.struct_size += 8; }, "struct_size long");
        with([](dsd_word_dur_args& a) { a.dur = nullptr; }, "null dur");
        with([](dsd_word_dur_args& a) { a.word_dur = nullptr; }, "null word_dur");
        with([](dsd_word_dur_args& a) { a.index = nullptr; }, "neither index nor slur");
        with([&](dsd_word_dur_args& a) { a.slur = u8.data(); }, "both index and slur");
        for (int B : {0, -1, 65536, INT32_MIN, INT32_MAX}) with([B](dsd_word_dur_args& a) { a.B = B; a.totals = nullptr; }, "bad B");
        for (int n : {0, -1, 2049, INT32_MIN, INT32_MAX}) {
            with([n](dsd_word_dur_args& a) { a.N = n; }, "bad N");
            with([n](dsd_word_dur_args& a) { a.W = n; }, "bad W");
        }
        for (int64_t t : {(int64_t)-1, (int64_t)INT32_MAX + 1, std::numeric_limits<int64_t>::min(), std::numeric_limits<int64_t>::max()}) {
            int64_t two[2] = {3, t};
            with([&](dsd_word_dur_args& a) { a.totals = two; }, "bad total");
        }
        dsd_word_dur_args edge = good;
        int64_t big[2] = {0, INT32_MAX};
        edge.totals = big;
        if (dsd_word_dur(0, &edge, nullptr) != DSD_OK) bad("totals 0 and 2^31 - 1 are allowed");
        g_launches_seen = g_launches;
    }
    // dsd_group_midi
    {
        dsd_group_midi_args good;
        memset(&good, 0, sizeof(good));
        good.struct_size = sizeof(good); good.B = 2; good.Nn = 3; good.G = 4; good.L = 5; good.T = 9;
        good.note_midi = f32.data(); good.note_dur = i64.data(); good.group_dur = i64.data(); good.ph2word = i64.data(); good.midi = i64.data() + 32;
        refused(dsd_group_midi(0, nullptr, nullptr), "null args");
        auto with = [&](auto change, const char* what) {
            dsd_group_midi_args a = good;
            change(a);
            refused(dsd_group_midi(0, &a, nullptr), what);
        };
        with([](dsd_group_midi_args& a) { a.struct_size = 0; }, "struct_size 0");
        with([](dsd_group_midi_args& a) { a.struct_size += 8; }, "struct_size long");
        with([](dsd_group_midi_args& a) { a.note_midi = nullptr; }, "null note_midi");
        with([](dsd_group_midi_args& a) { a.note_dur = nullptr; }, "null note_dur");
        with([](dsd_group_midi_args& a) { a.group_dur = nullptr; }, "null group_dur");
        with([](dsd_group_midi_args& a) { a.midi = nullptr; }, "null midi");
        with([](dsd_group_midi_args& a) { a.ph2word = nullptr; }, "L without ph2word");
        for (int B : {0, -1, 65536, INT32_MIN}) with([B](dsd_group_midi_args& a) { a.B = B; }, "bad B");
        for (int n : {0, -1, 2049, INT32_MIN, INT32_MAX}) {
            with([n](dsd_group_midi_args& a) { a.Nn = n; }, "bad Nn");
            with([n](dsd_group_midi_args& a) { a.G = n; }, "bad G");
            with([n](dsd_group_midi_args& a) { a.L = n; }, "bad L");
        }
        for (int t : {0, -1, INT32_MIN}) with([t](dsd_group_midi_args& a) { a.T = t; }, "bad T");
    }
    // dsd_rhythm_align
    {
        dsd_rhythm_align_args good;
        memset(&good, 0, sizeof(good));
        good.struct_size = sizeof(good); good.B = 2; good.L = 5; good.W = 3;
        good.ph_dur_pred = f32.data(); good.ph2word = i64.data(); good.word_dur = i64.data(); good.ph_dur = i64.data() + 32;
        refused(dsd_rhythm_align(0, nullptr, nullptr), "null args");
        auto with = [&](auto change, const char* what) {
            dsd_rhythm_align_args a = good;
            change(a);
            refused(dsd_rhythm_align(0, &a, nullptr), what);
        };
        with([](dsd_rhythm_align_args& a) { a.struct_size = 0; }, "struct_size 0");
        with([](dsd_rhythm_align_args& a) { a.struct_size -= 8; }, "struct_size short");
        with([](dsd_rhythm_align_args& a) { a.ph_dur_pred = nullptr; }, "null ph_dur_pred");
        with([](dsd_rhythm_align_args& a) { a.ph2word = nullptr; }, "null ph2word");
        with([](dsd_rhythm_align_args& a) { a.word_dur = nullptr; }, "null word_dur");
        with([](dsd_rhythm_align_args& a) { a.ph_dur = nullptr; }, "null ph_dur");
        for (int B : {0, -1, 65536, INT32_MIN}) with([B](dsd_rhythm_align_args& a) { a.B = B; }, "bad B");
        for (int n : {0, -1, 2049, INT32_MIN, INT32_MAX}) {
            with([n](dsd_rhythm_align_args& a) { a.L = n; }, "bad L");
            with([n](dsd_rhythm_align_args& a) { a.W = n; }, "bad W");
        }
    }

    printf("words_harness: %d calls run on exactly sized arrays, %d calls refused, %d unexpected results\n", g_ran, g_refused, g_bad);
    return g_bad ? 1 : 0;
}
