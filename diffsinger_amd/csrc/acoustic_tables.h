// Host-only checks behind dsd_acoustic_open (acoustic_tables.hip): a DSD_ACOUSTIC_TABLES section against its config and
// the inner sections' configs against it; dsd_acoustic_plan lives in the same file.  No HIP header:
// tools/harness/acoustic_harness.cpp links the same code under the host compiler's sanitizers.
#pragma once
#include <stdint.h>

#include "../../include/dsdenoise.h"

namespace dsd {

// where each table sits in `tensors` (an index, or -1 when the section has none)
struct AcousticTableIndex {
    int mask, spec_min, spec_max, pitch_embed, frozen_spk, frozen_key_shift;
    int mask_any;                                   // 1: the cross-lingual mask has a set entry
};

// the config's own rules, then every tensor it requires (by name and shape), none it excludes, the mask's values 0 / 1,
// spec_max[m] > spec_min[m].  `section` names the section in the message.  DSD_OK, or DSD_EINVAL through fail(nullptr, ...).
int acoustic_tables_check(const dsd_acoustic_config* cfg, int32_t cfg_size, const dsd_model_tensor_info* tensors, int32_t n_tensors,
                          const char* section, AcousticTableIndex* index);
// fs2: the acoustic encoder's config, denoiser: the backbone's, aux: the aux decoder's (nullptr without shallow diffusion)
int acoustic_inner_check(const dsd_acoustic_config* cfg, const dsd_encoder_config* fs2, const dsd_config* denoiser, const dsd_config* aux);

}  // namespace dsd
