// libdsdenoise, host side of the variance front end's score algebra: dsd_word_dur, dsd_group_midi, dsd_rhythm_align
// (kernels: words_kernels.hip).  Handle-free like dsd_length_regulate, whose frame assignment dsd_group_midi shares: no
// weights, no device memory of their own.
//
// Host code only, as curve_api.hip: no kernel, no HIP call, no HIP header.  Every argument check comes before the device is
// selected; the device selection is api.hip's and the launches are words_kernels.hip's, reached through plain functions.  So
// the same file compiles with a plain host compiler (tools/harness/words_harness.cpp builds it that way, under the
// sanitizers, with stand-ins for those functions).
#include <stdint.h>
#include <string.h>

#include "../../include/dsdenoise.h"
#include "words_params.h"

struct dsd_handle;
namespace dsd {
// api.hip: records the message for dsd_last_error(NULL) when h == nullptr and returns `code`
int fail(dsd_handle* h, int code, const char* fmt, ...);
int select_device(const char* who, int device, bool say_range);
}  // namespace dsd
using dsd::fail;

namespace {

constexpr int kMaxItems = 65535;        // the batch rides in the grid

int check_struct(const char* who, const void* args, int32_t struct_size, size_t want) {
    if (!args) return fail(nullptr, DSD_EINVAL, "%s: NULL args", who);
    if (struct_size != (int32_t)want) return fail(nullptr, DSD_EINVAL, "%s: struct_size %d != %zu", who, struct_size, want);
    return DSD_OK;
}
int check_batch(const char* who, int B) {
    if (B < 1 || B > kMaxItems) return fail(nullptr, DSD_EINVAL, "%s: B = %d outside [1, %d]", who, B, kMaxItems);
    return DSD_OK;
}
int check_count(const char* who, const char* name, int n) {
    if (n < 1 || n > dsd::kWordsMax) return fail(nullptr, DSD_EINVAL, "%s: %s = %d outside [1, %d]", who, name, n, dsd::kWordsMax);
    return DSD_OK;
}

}  // namespace

extern "C" {

int dsd_word_dur(int32_t device, const dsd_word_dur_args* a, void* stream) {
    const char* who = "dsd_word_dur";
    if (int rc = check_struct(who, a, a ? a->struct_size : 0, sizeof(*a))) return rc;
    if (!a->dur || !a->word_dur) return fail(nullptr, DSD_EINVAL, "%s: NULL dur or word_dur", who);
    if (!a->index == !a->slur)
        return fail(nullptr, DSD_EINVAL, "%s: exactly one of index and slur is given (%s)", who, a->index ? "both are set" : "both are NULL");
    if (int rc = check_batch(who, a->B)) return rc;
    if (int rc = check_count(who, "N", a->N)) return rc;
    if (int rc = check_count(who, "W", a->W)) return rc;
    if (a->totals)
        for (int b = 0; b < a->B; ++b)
            if (a->totals[b] < 0 || a->totals[b] > INT32_MAX)
                return fail(nullptr, DSD_EINVAL, "%s: totals[%d] = %lld outside [0, 2^31 - 1]", who, b, (long long)a->totals[b]);
    if (int rc = dsd::select_device(who, device, false)) return rc;
    dsd::WordDurP p;
    memset(&p, 0, sizeof(p));
    p.index = a->index; p.slur = a->slur; p.index_out = a->index_out;
    p.N = a->N; p.W = a->W;
    p.dur = a->dur; p.word_dur = a->word_dur;
    p.has_totals = a->totals != nullptr;
    const int step = a->totals ? dsd::kWordItems : a->B;       // the totals travel in the launch arguments, kWordItems at a time
    for (int b0 = 0; b0 < a->B; b0 += step) {
        const int items = a->B - b0 < step ? a->B - b0 : step;
        p.b0 = b0;
        if (a->totals)
            for (int k = 0; k < items; ++k) p.total[k] = (int32_t)a->totals[b0 + k];
        if (const char* err = dsd::launch_word_dur(p, items, stream)) return fail(nullptr, DSD_EHIP, "%s: launch failed: %s", who, err);
    }
    return DSD_OK;
}

int dsd_group_midi(int32_t device, const dsd_group_midi_args* a, void* stream) {
    const char* who = "dsd_group_midi";
    if (int rc = check_struct(who, a, a ? a->struct_size : 0, sizeof(*a))) return rc;
    if (!a->note_midi || !a->note_dur || !a->group_dur || !a->midi)
        return fail(nullptr, DSD_EINVAL, "%s: NULL note_midi, note_dur, group_dur or midi", who);
    if (int rc = check_batch(who, a->B)) return rc;
    if (int rc = check_count(who, "Nn", a->Nn)) return rc;
    if (int rc = check_count(who, "G", a->G)) return rc;
    if (a->ph2word) {
        if (int rc = check_count(who, "L", a->L)) return rc;
    } else if (a->L != 0) {
        return fail(nullptr, DSD_EINVAL, "%s: L = %d without ph2word (L is the length of ph2word; 0 without it)", who, a->L);
    }
    if (a->T < 1) return fail(nullptr, DSD_EINVAL, "%s: T = %d must be positive", who, a->T);
    if (int rc = dsd::select_device(who, device, false)) return rc;
    dsd::GroupMidiP p;
    memset(&p, 0, sizeof(p));
    p.note_midi = a->note_midi; p.note_dur = a->note_dur; p.group_dur = a->group_dur; p.ph2word = a->ph2word; p.midi = a->midi;
    p.Nn = a->Nn; p.G = a->G; p.L = a->L; p.T = a->T;
    if (const char* err = dsd::launch_group_midi(p, a->B, stream)) return fail(nullptr, DSD_EHIP, "%s: launch failed: %s", who, err);
    return DSD_OK;
}

int dsd_rhythm_align(int32_t device, const dsd_rhythm_align_args* a, void* stream) {
    const char* who = "dsd_rhythm_align";
    if (int rc = check_struct(who, a, a ? a->struct_size : 0, sizeof(*a))) return rc;
    if (!a->ph_dur_pred || !a->ph2word || !a->word_dur || !a->ph_dur)
        return fail(nullptr, DSD_EINVAL, "%s: NULL ph_dur_pred, ph2word, word_dur or ph_dur", who);
    if (int rc = check_batch(who, a->B)) return rc;
    if (int rc = check_count(who, "L", a->L)) return rc;
    if (int rc = check_count(who, "W", a->W)) return rc;
    if (int rc = dsd::select_device(who, device, false)) return rc;
    dsd::RhythmP p;
    memset(&p, 0, sizeof(p));
    p.pred = a->ph_dur_pred; p.ph2word = a->ph2word; p.word_dur = a->word_dur; p.out = a->ph_dur;
    p.L = a->L; p.W = a->W;
    if (const char* err = dsd::launch_rhythm_align(p, a->B, stream)) return fail(nullptr, DSD_EHIP, "%s: launch failed: %s", who, err);
    return DSD_OK;
}

}  // extern "C"
