// What words_api.hip (host code only, no HIP header) hands to words_kernels.hip: the checked arguments of dsd_word_dur,
// dsd_group_midi and dsd_rhythm_align as they travel in the launch arguments.  Plain C++, so the host file also compiles with
// a plain host compiler (tools/harness/words_harness.cpp).
#pragma once
#include <stdint.h>

namespace dsd {

constexpr int kWordsMax = 2048;     // kRegulateMaxTokens: the most phones, words or notes of a row
constexpr int kWordItems = 64;      // items of one dsd_word_dur launch that carries totals

struct WordDurP {
    const int64_t* dur;             // [B][N]
    const int64_t* index;           // [B][N], or
    const uint8_t* slur;            // [B][N]
    int64_t* word_dur;              // [B][W]
    int64_t* index_out;             // [B][N] or nullptr
    int32_t N, W, b0;               // the launch covers items b0 .. b0 + gridDim.x - 1
    int32_t has_totals;
    int32_t total[kWordItems];      // frames of item b0 + k (has_totals)
};

struct GroupMidiP {
    const float* note_midi;         // [B][Nn]
    const int64_t* note_dur;        // [B][Nn]
    const int64_t* group_dur;       // [B][G]
    const int64_t* ph2word;         // [B][L] or nullptr
    int64_t* midi;                  // [B][L] with ph2word, else [B][G]
    int32_t Nn, G, L, T;
};

struct RhythmP {
    const float* pred;              // [B][L]
    const int64_t* ph2word;         // [B][L]
    const int64_t* word_dur;        // [B][W]
    int64_t* out;                   // [B][L]
    int32_t L, W;
};

// words_kernels.hip: nullptr, or the text of the HIP error.  One launch each, of `items` workgroups.
const char* launch_word_dur(const WordDurP& p, int items, void* stream);
const char* launch_group_midi(const GroupMidiP& p, int items, void* stream);
const char* launch_rhythm_align(const RhythmP& p, int items, void* stream);

}  // namespace dsd
