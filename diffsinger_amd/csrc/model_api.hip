// libdsdenoise, from a model file to a handle: dsd_model_create.  Host code on top of the library's own public calls -
// the reader's accessors (model_file.hip), the nine create calls, dsd_load_weight and dsd_finalize_weights - so a handle
// made here is, call for call, the handle a C program would have made by hand from the same config and tensors.
#include <stdint.h>
#include <string.h>

#include <string>

#include "../../include/dsdenoise.h"

namespace dsd {
// api.hip: records the message for dsd_last_error(NULL) when h == nullptr and returns `code`
int fail(dsd_handle* h, int code, const char* fmt, ...);
}  // namespace dsd
using dsd::fail;

namespace {

// the largest config struct, suitably aligned for each of them
union AnyConfig {
    dsd_config backbone;
    dsd_encoder_config encoder;
    dsd_vocoder_config vocoder;
    dsd_token_encoder_config token_encoder;
    dsd_mel_config mel;
    dsd_rmvpe_config rmvpe;
    dsd_hnsep_config hnsep;
};

// puts `device` into the config and calls the create of the section's kind (kinds 0 .. 2: dsd_create_any_width, the call
// the Python shims make, so that every width the reference builds opens)
int create_kind(int32_t kind, AnyConfig& cfg, int32_t device, dsd_handle** out) {
    switch (kind) {
        case DSD_BACKBONE_WAVENET:
        case DSD_BACKBONE_LYNXNET:
        case DSD_AUX_CONVNEXT:
            cfg.backbone.device = device;
            return dsd_create_any_width(&cfg.backbone, out);
        case DSD_ENC_FS2_ACOUSTIC:
            cfg.encoder.device = device;
            return dsd_encoder_create(&cfg.encoder, out);
        case DSD_VOC_NSF_HIFIGAN:
            cfg.vocoder.device = device;
            return dsd_vocoder_create(&cfg.vocoder, out);
        case DSD_ENC_FS2_TOKENS:
            cfg.token_encoder.device = device;
            return dsd_token_encoder_create(&cfg.token_encoder, out);
        case DSD_MEL_ANALYSIS:
            cfg.mel.device = device;
            return dsd_mel_create(&cfg.mel, out);
        case DSD_PE_RMVPE:
            cfg.rmvpe.device = device;
            return dsd_rmvpe_create(&cfg.rmvpe, out);
        case DSD_HNSEP_VR:
            cfg.hnsep.device = device;
            return dsd_hnsep_create(&cfg.hnsep, out);
    }
    return fail(nullptr, DSD_EINVAL, "unknown kind %d", kind);       // dsd_model_open lets no such section through
}

}  // namespace

extern "C" int dsd_model_create(const dsd_model_file* f, int32_t section, int32_t device, dsd_handle** out) {
    const char* who = "dsd_model_create";
    if (out) *out = nullptr;
    if (!f || !out) return fail(nullptr, DSD_EINVAL, "%s: NULL argument", who);
    dsd_model_section_info info;
    int rc = dsd_model_section(f, section, &info);
    if (rc != DSD_OK) return fail(nullptr, rc, "%s: %s", who, std::string(dsd_last_error(nullptr)).c_str());
    if (info.kind == DSD_VARIANCE_TABLES)
        return fail(nullptr, DSD_EINVAL, "%s: section \"%s\" holds the variance model's tables, not a handle: open the model with dsd_variance_open",
                    who, info.name);
    if (info.kind == DSD_ACOUSTIC_TABLES)
        return fail(nullptr, DSD_EINVAL, "%s: section \"%s\" holds the acoustic model's tables, not a handle: use dsd_acoustic_open",
                    who, info.name);
    AnyConfig cfg;
    memset(&cfg, 0, sizeof(cfg));
    if (info.config_size < 0 || (size_t)info.config_size > sizeof(cfg))
        return fail(nullptr, DSD_EINVAL, "%s: section \"%s\": config of %d bytes", who, info.name, info.config_size);
    rc = dsd_model_config(f, section, &cfg, info.config_size);
    if (rc != DSD_OK) return fail(nullptr, rc, "%s: %s", who, std::string(dsd_last_error(nullptr)).c_str());

    dsd_handle* h = nullptr;
    rc = create_kind(info.kind, cfg, device, &h);
    if (rc != DSD_OK || !h) {
        const std::string why = dsd_last_error(nullptr);        // a copy: fail() below writes the buffer it points into
        if (h) dsd_destroy(h);
        return fail(nullptr, rc != DSD_OK ? rc : DSD_ESTATE, "%s: section \"%s\": %s", who, info.name, why.c_str());
    }
    if (info.kind == DSD_MEL_ANALYSIS) {     // no weights: dsd_load_weight and dsd_finalize_weights answer DSD_ESTATE on it
        *out = h;
        return DSD_OK;
    }
    for (int32_t j = 0; j < info.n_tensors; ++j) {
        dsd_model_tensor_info t;
        rc = dsd_model_tensor(f, section, j, &t);
        if (rc != DSD_OK) {
            const std::string why = dsd_last_error(nullptr);
            dsd_destroy(h);
            return fail(nullptr, rc, "%s: section \"%s\": %s", who, info.name, why.c_str());
        }
        rc = dsd_load_weight(h, t.name, t.data, t.shape, t.ndim, /*on_device=*/0);
        if (rc != DSD_OK) {
            const std::string why = dsd_last_error(h);
            dsd_destroy(h);
            return fail(nullptr, rc, "%s: section \"%s\", tensor \"%s\": %s", who, info.name, t.name, why.c_str());
        }
    }
    rc = dsd_finalize_weights(h);
    if (rc != DSD_OK) {
        const std::string why = dsd_last_error(h);
        dsd_destroy(h);
        return fail(nullptr, rc, "%s: section \"%s\": %s", who, info.name, why.c_str());
    }
    *out = h;
    return DSD_OK;
}
