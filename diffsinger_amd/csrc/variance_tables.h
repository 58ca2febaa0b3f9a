// Host-only checks behind dsd_variance_open (variance_tables.hip): a DSD_VARIANCE_TABLES section against its config, the
// inner sections' configs against it, and the smoothing taps.  No HIP header: tools/harness/variance_harness.cpp links
// the same code under the host compiler's sanitizers.
#pragma once
#include <stdint.h>

#include "../../include/dsdenoise.h"

namespace dsd {

// where each table sits in `tensors` (an index, or -1 when the model has none)
struct VarianceTableIndex {
    int txt, mask, lang, onset, dur_w, dur_b, midi, spk;
    int note_midi_w, note_midi_b, note_dur_w, note_dur_b, glide;
    int retake, pitch_in_w, pitch_in_b;             // delta_pitch_embed or base_pitch_embed
    int pitch_w, pitch_b;
    int taps;                                       // smooth_taps: optional with predict_pitch (-1: computed at open)
    int var_w[DSD_VAR_MAX_CURVES], var_b[DSD_VAR_MAX_CURVES];      // in checklist order, -1 where the bit is clear
    int mask_any;                                   // 1: the cross-lingual mask has a set entry
};

extern const char* const kVarianceNames[DSD_VAR_MAX_CURVES];

// the config's own rules, then every tensor the flags require (by name and shape), none they exclude, the mask's values
// 0 / 1.  `section` names the section in the message.  DSD_OK, or DSD_EINVAL through fail(nullptr, ...).
int variance_tables_check(const dsd_variance_config* cfg, int32_t cfg_size, const dsd_model_tensor_info* tensors, int32_t n_tensors,
                          const char* section, VarianceTableIndex* index);
// fs2 / melody: token encoder configs, pitch / variances: denoiser configs; nullptr where the model has no such section
int variance_inner_check(const dsd_variance_config* cfg, const dsd_token_encoder_config* fs2, const dsd_token_encoder_config* melody,
                         const dsd_config* pitch, const dsd_config* variances);
// build_smooth_op's taps (toplevel.py:189-192) for K in [1, 255]: w[k] = sin(pi * linspace(0, 1, K)[k]) / sum
void variance_smooth_taps(int K, float* w);
inline int variance_count(uint32_t bits) {
    int n = 0;
    for (int i = 0; i < DSD_VAR_MAX_CURVES; ++i) n += (bits >> i) & 1u;
    return n;
}

}  // namespace dsd
