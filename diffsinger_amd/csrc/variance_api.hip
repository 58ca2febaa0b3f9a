// libdsdenoise, the variance model's staged twin on one model file: dsd_variance_open / _close / _info / _backbone and the
// six stage calls.  Host code on top of the library's own public calls - the model file reader, dsd_model_create,
// dsd_length_regulate, dsd_frame_curve, dsd_cond_assemble, dsd_token_encode, dsd_predict_dur - plus the launches of
// stage_kernels.hip.  The gathers and terms of every assemble call stand in the order diffsinger_amd/deploy.py gives them,
// so a stage's output is bit-identical to the Python twin's on the same operands.  The host-only checks of a tables
// section are variance_tables.hip.
#include "api_host.h"
#include "variance_tables.h"

struct dsd_variance {
    dsd_variance_config cfg;
    int device = 0;
    VarianceTableIndex ix;
    bool lang_on = false;               // use_lang_id and a set entry in the cross-lingual mask
    int n_var = 0;
    int var_slot[DSD_VAR_MAX_CURVES];   // the i-th predicted variance's place in the checklist
    dsd_handle *fs2 = nullptr, *melody = nullptr, *pitch = nullptr, *variances = nullptr;
    DevBuf<float> tables;               // every tensor of the tables section, in file order
    std::vector<size_t> off;            // float offset of tensor j
    float taps[kCurveMaxTaps];
    // one workspace per stage, grown on demand: a call at sizes already met allocates nothing, and a graph captured over a
    // stage stays valid until that stage is called with larger sizes
    DevBuf<char> ws_encode, ws_dur, ws_pitch, ws_cond;
    SpkMixIds spk_ids;                  // dsd_variance_spk_mix's ids on the device
    // dsd_variance_set_lengths: the lengths the frame-level stage calls check their (B, T) against and dsd_frame_curve takes;
    // the two denoisers hold their own copies
    bool ragged = false;
    std::vector<int32_t> lengths;
    const float* tab(int j) const { return tables.p + off[(size_t)j]; }
    ~dsd_variance() {
        for (dsd_handle* h : {fs2, melody, pitch, variances})
            if (h) dsd_destroy(h);
    }
};

namespace {

constexpr int kMaxItems = 65535;        // the batch rides in gridDim.y

// carves a stage's workspace: sizes first (p == nullptr), then the pointers
struct Carver {
    char* p;
    size_t used = 0;
    explicit Carver(char* base) : p(base) {}
    template <typename T>
    T* take(size_t n) {
        used = (used + 255) & ~(size_t)255;
        T* out = p ? reinterpret_cast<T*>(p + used) : nullptr;
        used += n * sizeof(T);
        return out;
    }
};

std::string last(dsd_handle* h) { return std::string(dsd_last_error(h)); }

#define LIB_OK(who, call, what)                                                                  \
    do {                                                                                         \
        const int rc_ = (call);                                                                  \
        if (rc_ != DSD_OK) return fail(nullptr, rc_, "%s: %s: %s", who, what, last(nullptr).c_str()); \
    } while (0)
#define HANDLE_OK(who, h, call, what)                                                            \
    do {                                                                                         \
        const int rc_ = (call);                                                                  \
        if (rc_ != DSD_OK) return fail(nullptr, rc_, "%s: %s: %s", who, what, last(h).c_str());  \
    } while (0)
#define LAUNCH_OK(who, call, what)                                                               \
    do {                                                                                         \
        const hipError_t e_ = (call);                                                            \
        if (e_ != hipSuccess) return fail(nullptr, DSD_EHIP, "%s: %s launch failed: %s", who, what, hipGetErrorString(e_)); \
    } while (0)

int check_sizes(const char* who, int B, int L, int W, int N, int T) {
    if (B < 1 || B > kMaxItems) return fail(nullptr, DSD_EINVAL, "%s: B = %d outside [1, %d]", who, B, kMaxItems);
    if (L != -1 && (L < 1 || L > kRegulateMaxTokens)) return fail(nullptr, DSD_EINVAL, "%s: L = %d outside [1, %d]", who, L, kRegulateMaxTokens);
    if (W != -1 && (W < 1 || W > kRegulateMaxTokens)) return fail(nullptr, DSD_EINVAL, "%s: W = %d outside [1, %d]", who, W, kRegulateMaxTokens);
    if (N != -1 && (N < 1 || N > kRegulateMaxTokens)) return fail(nullptr, DSD_EINVAL, "%s: N = %d outside [1, %d]", who, N, kRegulateMaxTokens);
    if (T != -1 && T < 1) return fail(nullptr, DSD_EINVAL, "%s: T = %d must be positive", who, T);
    if (T != -1 && (int64_t)B * T > INT32_MAX) return fail(nullptr, DSD_EINVAL, "%s: B * T = %lld exceeds 2^31 - 1", who, (long long)B * T);
    return DSD_OK;
}

int check_spk(const char* who, const dsd_variance* v, const float* spk_embed, int rows, int len, const char* len_name) {
    if (!spk_embed) return DSD_OK;
    if (!v->cfg.use_spk_id) return fail(nullptr, DSD_EINVAL, "%s: spk_embed given, but the model has no speaker embedding (use_spk_id = 0)", who);
    if (rows != 1 && rows != len) return fail(nullptr, DSD_EINVAL, "%s: spk_rows = %d is neither 1 nor %s = %d", who, rows, len_name, len);
    return DSD_OK;
}

void init_assemble(dsd_assemble_args& a, const dsd_variance* v, int B, int T, int H) {
    memset(&a, 0, sizeof(a));
    a.struct_size = sizeof(a);
    a.device = v->device;
    a.B = B; a.T = T; a.H = H;
}
void add_gather(dsd_assemble_args& a, const float* table, int64_t batch_stride, int64_t rows, const int64_t* idx, int64_t offset, float scale) {
    auto& g = a.gather[a.n_gather++];
    g.table = table; g.batch_stride = batch_stride; g.rows = rows; g.idx = idx; g.idx_offset = offset; g.scale = scale; g.row_scale = nullptr;
}
void add_term(dsd_assemble_args& a, const float* s, const float* vec) {
    a.term[a.n_terms].s = s;
    a.term[a.n_terms++].v = vec;
}
// the speaker gather of deploy.py's _spk_gather: [B, rows, H] at index t (rows == len > 1) or 0
void add_spk(dsd_assemble_args& a, const float* spk_embed, int rows, int H, const int64_t* spk_idx) {
    add_gather(a, spk_embed, (int64_t)rows * H, rows, spk_idx, 0, 1.0f);
}

// dsd_set_lengths' rules for the frame-level stage calls, checked by the object itself: none of them reaches a denoiser that would
int check_lengths(const dsd_variance* v, const char* who, int B, int T) {
    if (!v->ragged) return DSD_OK;
    if ((int)v->lengths.size() != B)
        return fail(nullptr, DSD_ESTATE, "%s: dsd_variance_set_lengths gave %d lengths but this call runs a batch of %d", who,
                    (int)v->lengths.size(), B);
    for (int b = 0; b < B; ++b)
        if (v->lengths[(size_t)b] > T) return fail(nullptr, DSD_EINVAL, "%s: lengths[%d] = %d exceeds T = %d", who, b, v->lengths[(size_t)b], T);
    return DSD_OK;
}

int section_of(const dsd_model_file* f, const std::string& name, const char* who, bool tables, dsd_model_section_info* info) {
    const int i = dsd_model_find(f, name.c_str());
    if (i < 0) return fail(nullptr, DSD_ENOTFOUND, "%s: the file has no section \"%s\"", who, name.c_str());
    if (int rc = dsd_model_section(f, i, info)) return rc;
    if (tables && info->kind != DSD_VARIANCE_TABLES)
        return fail(nullptr, DSD_EINVAL, "%s: section \"%s\" is of kind %d, not DSD_VARIANCE_TABLES (%d)", who, name.c_str(), info->kind, DSD_VARIANCE_TABLES);
    return i + 1;       // > 0: the index plus one
}

int open_impl(const dsd_model_file* f, const char* prefix, int32_t device, dsd_variance* v) {
    const char* who = "dsd_variance_open";
    const std::string pre(prefix);
    dsd_model_section_info info;
    int rc = section_of(f, pre + ".tables", who, true, &info);
    if (rc < 0) return rc;
    const int tables_i = rc - 1;
    if (info.config_size != (int32_t)sizeof(dsd_variance_config))
        return fail(nullptr, DSD_EINVAL, "%s: section \"%s\": config of %d bytes", who, info.name, info.config_size);
    LIB_OK(who, dsd_model_config(f, tables_i, &v->cfg, info.config_size), "the tables' config");
    std::vector<dsd_model_tensor_info> tensors((size_t)info.n_tensors);
    for (int32_t j = 0; j < info.n_tensors; ++j) LIB_OK(who, dsd_model_tensor(f, tables_i, j, &tensors[(size_t)j]), "a table");
    if (int r = variance_tables_check(&v->cfg, info.config_size, tensors.data(), info.n_tensors, info.name, &v->ix)) return r;
    const dsd_variance_config& c = v->cfg;
    v->lang_on = c.use_lang_id && v->ix.mask_any;
    for (int i = 0; i < DSD_VAR_MAX_CURVES; ++i)
        if ((c.variances >> i) & 1u) v->var_slot[v->n_var++] = i;

    // the inner sections: kinds and configs, still on the host
    struct Inner {
        const char* suffix;
        bool wanted, encoder;
        int index = -1;
        dsd_token_encoder_config tcfg;
        dsd_config dcfg;
    } inner[4] = {{".fs2", true, true}, {".melody", c.use_melody_encoder != 0, true}, {".pitch", c.predict_pitch != 0, false},
                  {".variances", c.variances != 0, false}};
    for (Inner& in : inner) {
        if (!in.wanted) continue;
        dsd_model_section_info si;
        rc = section_of(f, pre + in.suffix, who, false, &si);
        if (rc < 0) return rc;
        in.index = rc - 1;
        if (in.encoder) {
            if (si.kind != DSD_ENC_FS2_TOKENS)
                return fail(nullptr, DSD_EINVAL, "%s: section \"%s\" is of kind %d, not a token encoder (%d)", who, si.name, si.kind, DSD_ENC_FS2_TOKENS);
            LIB_OK(who, dsd_model_config(f, in.index, &in.tcfg, sizeof(in.tcfg)), si.name);
        } else {
            if (si.kind != DSD_BACKBONE_WAVENET && si.kind != DSD_BACKBONE_LYNXNET)
                return fail(nullptr, DSD_EINVAL, "%s: section \"%s\" is of kind %d, not a denoiser (%d or %d)", who, si.name, si.kind,
                            DSD_BACKBONE_WAVENET, DSD_BACKBONE_LYNXNET);
            LIB_OK(who, dsd_model_config(f, in.index, &in.dcfg, sizeof(in.dcfg)), si.name);
        }
    }
    if (int r = variance_inner_check(&c, &inner[0].tcfg, inner[1].wanted ? &inner[1].tcfg : nullptr, inner[2].wanted ? &inner[2].dcfg : nullptr,
                                     inner[3].wanted ? &inner[3].dcfg : nullptr))
        return r;
    if (c.predict_pitch) {          // the file's taps (what the exporter's build_smooth_op computed), else the library's own
        if (v->ix.taps >= 0) memcpy(v->taps, tensors[(size_t)v->ix.taps].data, sizeof(float) * (size_t)c.smooth_width);
        else variance_smooth_taps(c.smooth_width, v->taps);
    }

    // the device: inner handles, then the tables in one block
    if (int r = select_device(who, device)) return r;
    v->device = device;
    dsd_handle** slots[4] = {&v->fs2, &v->melody, &v->pitch, &v->variances};
    for (int k = 0; k < 4; ++k)
        if (inner[k].wanted) LIB_OK(who, dsd_model_create(f, inner[k].index, device, slots[k]), "an inner handle");
    std::vector<float> host;
    v->off.resize(tensors.size());
    for (size_t j = 0; j < tensors.size(); ++j) {
        v->off[j] = host.size();
        host.insert(host.end(), tensors[j].data, tensors[j].data + tensors[j].count);
        host.resize((host.size() + 63) / 64 * 64, 0.f);
    }
    if (int r = v->tables.reserve(nullptr, host.size(), who)) return r;
    HIP_OK(nullptr, hipMemcpy(v->tables.p, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice));
    return DSD_OK;
}

int enter_stage(const char* who, dsd_variance* v, const void* args, int32_t struct_size, size_t want_size) {
    if (!v) return fail(nullptr, DSD_EINVAL, "%s: NULL object", who);
    if (!args) return fail(nullptr, DSD_EINVAL, "%s: NULL args", who);
    if (struct_size != (int32_t)want_size) return fail(nullptr, DSD_EINVAL, "%s: struct_size %d != %zu", who, struct_size, want_size);
    return DSD_OK;
}

}  // namespace

extern "C" {

int dsd_variance_open(const dsd_model_file* f, const char* prefix, int32_t device, dsd_variance** out) {
    const char* who = "dsd_variance_open";
    if (out) *out = nullptr;
    if (!f || !prefix || !out) return fail(nullptr, DSD_EINVAL, "%s: NULL argument", who);
    if (strlen(prefix) > DSD_MODEL_MAX_NAME - 10) return fail(nullptr, DSD_EINVAL, "%s: the prefix is longer than %d bytes", who, DSD_MODEL_MAX_NAME - 10);
    dsd_variance* v = nullptr;
    int rc;
    try {
        v = new dsd_variance();
        memset(&v->cfg, 0, sizeof(v->cfg));
        rc = open_impl(f, prefix, device, v);
    } catch (const std::exception&) {
        rc = fail(nullptr, DSD_ENOMEM, "%s: out of host memory", who);
    }
    if (rc != DSD_OK) {
        const std::string why = last(nullptr);      // the destructor's calls must not replace the message
        delete v;
        return fail(nullptr, rc, "%s", why.c_str());
    }
    *out = v;
    return DSD_OK;
}

void dsd_variance_close(dsd_variance* v) { delete v; }

int dsd_variance_info(const dsd_variance* v, dsd_variance_config* out) {
    if (!v || !out) return fail(nullptr, DSD_EINVAL, "dsd_variance_info: NULL argument");
    *out = v->cfg;
    return DSD_OK;
}

int dsd_variance_backbone(const dsd_variance* v, int32_t which, dsd_handle** out) {
    const char* who = "dsd_variance_backbone";
    if (out) *out = nullptr;
    if (!v || !out) return fail(nullptr, DSD_EINVAL, "%s: NULL argument", who);
    if (which != DSD_VAR_PITCH && which != DSD_VAR_VARIANCES) return fail(nullptr, DSD_EINVAL, "%s: which = %d is neither DSD_VAR_PITCH nor DSD_VAR_VARIANCES", who, which);
    dsd_handle* h = which == DSD_VAR_PITCH ? v->pitch : v->variances;
    if (!h) return fail(nullptr, DSD_EINVAL, "%s: the model has no %s predictor", who, which == DSD_VAR_PITCH ? "pitch" : "variance");
    *out = h;
    return DSD_OK;
}

int dsd_variance_encode(dsd_variance* v, const dsd_variance_encode_args* a, void* stream) {
    const char* who = "dsd_variance_encode";
    if (int rc = enter_stage(who, v, a, a ? a->struct_size : 0, sizeof(*a))) return rc;
    const dsd_variance_config& c = v->cfg;
    const bool word = c.predict_dur != 0;
    if (word && a->ph_dur)
        return fail(nullptr, DSD_EINVAL, "%s: the model is of the word form (predict_dur): ph_dur is the phoneme form's input", who);
    if (word && (!a->word_div || !a->word_dur)) return fail(nullptr, DSD_EINVAL, "%s: NULL word_div or word_dur", who);
    if (!word && (a->W != 0 || a->word_div || a->word_dur))
        return fail(nullptr, DSD_EINVAL, "%s: the model is of the phoneme form (no predict_dur): word_div / word_dur / W are the word form's inputs", who);
    if (!word && a->ph2word)
        return fail(nullptr, DSD_EINVAL, "%s: the model is of the phoneme form (no predict_dur): it has no ph2word to write", who);
    if (!word && !a->ph_dur) return fail(nullptr, DSD_EINVAL, "%s: NULL ph_dur", who);
    if (!a->tokens || !a->encoder_out || !a->x_masks) return fail(nullptr, DSD_EINVAL, "%s: NULL tokens, encoder_out or x_masks", who);
    if (int rc = check_sizes(who, a->B, a->L, word ? a->W : -1, -1, -1)) return rc;
    if (v->lang_on && !a->languages)
        return fail(nullptr, DSD_EINVAL, "%s: languages is required: the model's cross-lingual mask has a set entry", who);
    const int B = a->B, L = a->L, H = c.hidden_size;
    const size_t n = (size_t)B * L;
    HIP_OK(nullptr, hipSetDevice(v->device));       // before the workspace is sized: it lives on the object's device
    for (int pass = 0; pass < 2; ++pass) {
        Carver cv(pass ? v->ws_encode.p : nullptr);
        int64_t* ph2word = cv.take<int64_t>(n);
        int64_t* onset = cv.take<int64_t>(n);
        int64_t* lang = cv.take<int64_t>(n);
        float* dur_f = cv.take<float>(n);
        float* embed = cv.take<float>(n * H);
        if (!pass) {
            if (int rc = v->ws_encode.reserve(nullptr, cv.used, who)) return rc;
            continue;
        }
        hipStream_t st = (hipStream_t)stream;
        if (a->ph2word) ph2word = a->ph2word;
        if (word) LIB_OK(who, dsd_length_regulate(v->device, a->word_div, B, a->W, L, ph2word, stream), "ph2word");
        StageEncodeP p;
        memset(&p, 0, sizeof(p));
        p.tokens = (const long long*)a->tokens;
        p.ph2word = word ? (const long long*)ph2word : nullptr;
        p.word_dur = (const long long*)a->word_dur;
        p.ph_dur = (const long long*)a->ph_dur;
        p.languages = v->lang_on ? (const long long*)a->languages : nullptr;
        p.mask = v->tab(v->ix.mask);
        p.L = L; p.W = word ? a->W : 0; p.vocab = c.vocab_size;
        p.onset = (long long*)onset; p.lang = (long long*)lang; p.dur_f = dur_f; p.x_masks = a->x_masks;
        LAUNCH_OK(who, launch_stage_encode(p, B, st), "the index kernel");
        dsd_assemble_args as;
        init_assemble(as, v, B, L, H);
        add_gather(as, v->tab(v->ix.txt), 0, c.vocab_size, a->tokens, 0, (float)sqrt((double)H));
        if (word) add_gather(as, v->tab(v->ix.onset), 0, 2, onset, 0, 1.0f);
        if (v->lang_on) add_gather(as, v->tab(v->ix.lang), 0, (int64_t)c.num_lang + 1, lang, 0, 1.0f);
        add_term(as, dur_f, v->tab(v->ix.dur_w));
        add_term(as, nullptr, v->tab(v->ix.dur_b));
        LIB_OK(who, dsd_cond_assemble(&as, embed, stream), "the token embedding");
        HANDLE_OK(who, v->fs2, dsd_token_encode(v->fs2, embed, a->x_masks, B, L, a->encoder_out, stream), "the encoder");
    }
    return DSD_OK;
}

int dsd_variance_dur(dsd_variance* v, const dsd_variance_dur_args* a, void* stream) {
    const char* who = "dsd_variance_dur";
    if (int rc = enter_stage(who, v, a, a ? a->struct_size : 0, sizeof(*a))) return rc;
    const dsd_variance_config& c = v->cfg;
    if (!c.predict_dur) return fail(nullptr, DSD_EINVAL, "%s: the model has no duration predictor (predict_dur = 0)", who);
    if (!a->encoder_out || !a->x_masks || !a->ph_midi || !a->ph_dur_pred) return fail(nullptr, DSD_EINVAL, "%s: NULL encoder_out, x_masks, ph_midi or ph_dur_pred", who);
    if (int rc = check_sizes(who, a->B, a->L, -1, -1, -1)) return rc;
    if (int rc = check_spk(who, v, a->spk_embed, a->spk_rows, a->L, "L")) return rc;
    const int B = a->B, L = a->L, H = c.hidden_size;
    const size_t n = (size_t)B * L;
    HIP_OK(nullptr, hipSetDevice(v->device));       // before the workspace is sized: it lives on the object's device
    for (int pass = 0; pass < 2; ++pass) {
        Carver cv(pass ? v->ws_dur.p : nullptr);
        int64_t* iota = cv.take<int64_t>(n);
        int64_t* spk_idx = cv.take<int64_t>(n);
        float* dur_cond = cv.take<float>(n * H);
        if (!pass) {
            if (int rc = v->ws_dur.reserve(nullptr, cv.used, who)) return rc;
            continue;
        }
        LAUNCH_OK(who, launch_stage_iota((long long*)iota, a->spk_embed ? (long long*)spk_idx : nullptr, a->spk_rows == L && L > 1, B, L,
                                         (hipStream_t)stream), "the index kernel");
        dsd_assemble_args as;
        init_assemble(as, v, B, L, H);
        add_gather(as, a->encoder_out, (int64_t)L * H, L, iota, 0, 1.0f);
        add_gather(as, v->tab(v->ix.midi), 0, 128, a->ph_midi, 0, 1.0f);
        if (a->spk_embed) add_spk(as, a->spk_embed, a->spk_rows, H, spk_idx);
        LIB_OK(who, dsd_cond_assemble(&as, dur_cond, stream), "the duration condition");
        HANDLE_OK(who, v->fs2, dsd_predict_dur(v->fs2, dur_cond, a->x_masks, B, L, a->ph_dur_pred, stream), "the duration predictor");
    }
    return DSD_OK;
}

int dsd_variance_pitch_cond(dsd_variance* v, const dsd_variance_pitch_cond_args* a, void* stream) {
    const char* who = "dsd_variance_pitch_cond";
    if (int rc = enter_stage(who, v, a, a ? a->struct_size : 0, sizeof(*a))) return rc;
    const dsd_variance_config& c = v->cfg;
    if (!c.predict_pitch) return fail(nullptr, DSD_EINVAL, "%s: the model has no pitch predictor (predict_pitch = 0)", who);
    const bool mel = c.use_melody_encoder != 0;
    if (!a->encoder_out || !a->ph_dur || !a->note_midi || !a->note_dur || !a->pitch || !a->retake || !a->pitch_cond || !a->base_pitch)
        return fail(nullptr, DSD_EINVAL, "%s: NULL encoder_out, ph_dur, note_midi, note_dur, pitch, retake, pitch_cond or base_pitch", who);
    if (mel && !a->note_rest) return fail(nullptr, DSD_EINVAL, "%s: NULL note_rest on a model with a melody encoder", who);
    if (a->note_glide && !c.use_glide_embed) return fail(nullptr, DSD_EINVAL, "%s: note_glide given, but the model has no glide embedding (use_glide_embed = 0)", who);
    if (int rc = check_sizes(who, a->B, a->L, -1, a->N, a->T)) return rc;
    if (int rc = check_spk(who, v, a->spk_embed, a->spk_rows, a->T, "T")) return rc;
    if (a->lengths)
        for (int b = 0; b < a->B; ++b)
            if (a->lengths[b] < 0 || a->lengths[b] > a->T)
                return fail(nullptr, DSD_EINVAL, "%s: lengths[%d] = %d outside [0, T = %d]", who, b, a->lengths[b], a->T);
    if (int rc = check_lengths(v, who, a->B, a->T)) return rc;
    if (v->ragged && a->lengths)
        for (int b = 0; b < a->B; ++b)
            if (a->lengths[b] != v->lengths[(size_t)b])
                return fail(nullptr, DSD_EINVAL, "%s: lengths[%d] = %d, but dsd_variance_set_lengths gave %d", who, b, a->lengths[b],
                            v->lengths[(size_t)b]);
    const int32_t* lengths = v->ragged ? v->lengths.data() : a->lengths;
    const int B = a->B, L = a->L, N = a->N, T = a->T, H = c.hidden_size, Hm = c.melody_hidden_size;
    const size_t nt = (size_t)B * T, nn = (size_t)B * N;
    HIP_OK(nullptr, hipSetDevice(v->device));       // before the workspace is sized: it lives on the object's device
    for (int pass = 0; pass < 2; ++pass) {
        Carver cv(pass ? v->ws_pitch.p : nullptr);
        int64_t* mel2ph = cv.take<int64_t>(nt);
        int64_t* mel2note = cv.take<int64_t>(nt);
        int64_t* spk_idx = cv.take<int64_t>(nt);
        int64_t* glide = cv.take<int64_t>(nn);
        float* midi_s = cv.take<float>(nn);
        float* keep_s = cv.take<float>(nn);
        float* dur_f = cv.take<float>(nn);
        float* note_embed = cv.take<float>(mel ? nn * Hm : 0);
        float* melody_out = cv.take<float>(mel ? nn * H : 0);
        float* e = cv.take<float>(nt);
        float* one_minus_e = cv.take<float>(nt);
        float* other_a = cv.take<float>(nt);
        float* other_b = cv.take<float>(nt);
        uint8_t* pad = cv.take<uint8_t>(nn);
        if (!pass) {
            if (int rc = v->ws_pitch.reserve(nullptr, cv.used, who)) return rc;
            continue;
        }
        hipStream_t st = (hipStream_t)stream;
        LIB_OK(who, dsd_length_regulate(v->device, a->ph_dur, B, L, T, mel2ph, stream), "mel2ph");
        LIB_OK(who, dsd_length_regulate(v->device, a->note_dur, B, N, T, mel2note, stream), "mel2note");
        if (mel) {
            StageNoteP p;
            memset(&p, 0, sizeof(p));
            p.note_midi = a->note_midi; p.note_rest = a->note_rest; p.note_dur = (const long long*)a->note_dur;
            p.note_glide = (const long long*)a->note_glide;
            p.N = N; p.scale = (float)sqrt((double)Hm);
            p.midi_s = midi_s; p.keep_s = keep_s; p.dur_f = dur_f; p.glide = (long long*)glide; p.pad = pad;
            LAUNCH_OK(who, launch_stage_notes(p, B, st), "the note kernel");
            dsd_assemble_args as;
            init_assemble(as, v, B, N, Hm);
            if (c.use_glide_embed) add_gather(as, v->tab(v->ix.glide), 0, c.glide_rows, glide, 0, c.glide_embed_scale);
            add_term(as, midi_s, v->tab(v->ix.note_midi_w));
            add_term(as, keep_s, v->tab(v->ix.note_midi_b));
            add_term(as, dur_f, v->tab(v->ix.note_dur_w));
            add_term(as, nullptr, v->tab(v->ix.note_dur_b));
            LIB_OK(who, dsd_cond_assemble(&as, note_embed, stream), "the note embedding");
            HANDLE_OK(who, v->melody, dsd_token_encode(v->melody, note_embed, pad, B, N, melody_out, stream), "the melody encoder");
        }
        StageFrameP fp;
        memset(&fp, 0, sizeof(fp));
        fp.T = T; fp.V = 0; fp.expr = a->expr; fp.retake = a->retake; fp.e = e; fp.one_minus_e = one_minus_e;
        fp.spk_idx = a->spk_embed ? (long long*)spk_idx : nullptr;
        fp.spk_iota = a->spk_rows == T && T > 1;
        LAUNCH_OK(who, launch_stage_frames(fp, B, st), "the frame kernel");
        // base: the smoothed curve (with a melody encoder, the stage's second output); blend: the base pitch without one
        float* base = mel ? a->base_pitch : other_a;
        float* blend = mel ? other_a : a->base_pitch;
        float* delta = other_b;
        LIB_OK(who, dsd_frame_curve(v->device, a->note_midi, mel2note, a->pitch, a->retake, B, N, T, lengths, v->taps, c.smooth_width, base,
                                    blend, delta, stream), "the base pitch");
        dsd_assemble_args as;
        init_assemble(as, v, B, T, H);
        add_gather(as, a->encoder_out, (int64_t)L * H, L, mel2ph, -1, 1.0f);
        if (mel) add_gather(as, melody_out, (int64_t)N * H, N, mel2note, -1, 1.0f);
        if (a->spk_embed) add_spk(as, a->spk_embed, a->spk_rows, H, spk_idx);
        const float* emb = v->tab(v->ix.retake);
        add_term(as, e, emb + H);
        add_term(as, one_minus_e, emb);
        add_term(as, mel ? delta : blend, v->tab(v->ix.pitch_in_w));
        add_term(as, nullptr, v->tab(v->ix.pitch_in_b));
        LIB_OK(who, dsd_cond_assemble(&as, a->pitch_cond, stream), "the pitch condition");
    }
    return DSD_OK;
}

int dsd_variance_cond(dsd_variance* v, const dsd_variance_cond_args* a, void* stream) {
    const char* who = "dsd_variance_cond";
    if (int rc = enter_stage(who, v, a, a ? a->struct_size : 0, sizeof(*a))) return rc;
    const dsd_variance_config& c = v->cfg;
    if (!c.variances) return fail(nullptr, DSD_EINVAL, "%s: the model predicts no variance (variances = 0)", who);
    if (!a->encoder_out || !a->ph_dur || !a->pitch || !a->retake || !a->variance_cond)
        return fail(nullptr, DSD_EINVAL, "%s: NULL encoder_out, ph_dur, pitch, retake or variance_cond", who);
    for (int i = 0; i < v->n_var; ++i)
        if (!a->curves[i]) return fail(nullptr, DSD_EINVAL, "%s: NULL curves[%d] (%s)", who, i, kVarianceNames[v->var_slot[i]]);
    if (int rc = check_sizes(who, a->B, a->L, -1, -1, a->T)) return rc;
    if (int rc = check_spk(who, v, a->spk_embed, a->spk_rows, a->T, "T")) return rc;
    if (int rc = check_lengths(v, who, a->B, a->T)) return rc;
    const int B = a->B, L = a->L, T = a->T, H = c.hidden_size, V = v->n_var;
    const size_t nt = (size_t)B * T;
    HIP_OK(nullptr, hipSetDevice(v->device));       // before the workspace is sized: it lives on the object's device
    for (int pass = 0; pass < 2; ++pass) {
        Carver cv(pass ? v->ws_cond.p : nullptr);
        int64_t* mel2ph = cv.take<int64_t>(nt);
        int64_t* spk_idx = cv.take<int64_t>(nt);
        float *keep[DSD_VAR_MAX_CURVES], *kept[DSD_VAR_MAX_CURVES];
        for (int i = 0; i < V; ++i) {
            keep[i] = cv.take<float>(nt);
            kept[i] = cv.take<float>(nt);
        }
        if (!pass) {
            if (int rc = v->ws_cond.reserve(nullptr, cv.used, who)) return rc;
            continue;
        }
        LIB_OK(who, dsd_length_regulate(v->device, a->ph_dur, B, L, T, mel2ph, stream), "mel2ph");
        StageFrameP fp;
        memset(&fp, 0, sizeof(fp));
        fp.T = T; fp.V = V; fp.retake = a->retake;
        for (int i = 0; i < V; ++i) { fp.curves[i] = a->curves[i]; fp.keep[i] = keep[i]; fp.kept[i] = kept[i]; }
        fp.spk_idx = a->spk_embed ? (long long*)spk_idx : nullptr;
        fp.spk_iota = a->spk_rows == T && T > 1;
        LAUNCH_OK(who, launch_stage_frames(fp, B, (hipStream_t)stream), "the frame kernel");
        dsd_assemble_args as;
        init_assemble(as, v, B, T, H);
        add_gather(as, a->encoder_out, (int64_t)L * H, L, mel2ph, -1, 1.0f);
        if (a->spk_embed) add_spk(as, a->spk_embed, a->spk_rows, H, spk_idx);
        add_term(as, a->pitch, v->tab(v->ix.pitch_w));
        add_term(as, nullptr, v->tab(v->ix.pitch_b));
        for (int i = 0; i < V; ++i) {
            add_term(as, kept[i], v->tab(v->ix.var_w[v->var_slot[i]]));
            add_term(as, keep[i], v->tab(v->ix.var_b[v->var_slot[i]]));
        }
        LIB_OK(who, dsd_cond_assemble(&as, a->variance_cond, stream), "the variance condition");
    }
    return DSD_OK;
}

int dsd_variance_pitch_post(dsd_variance* v, const float* sample, const float* base_pitch, int32_t B, int32_t T, float* pitch_pred,
                            void* stream) {
    const char* who = "dsd_variance_pitch_post";
    if (!v) return fail(nullptr, DSD_EINVAL, "%s: NULL object", who);
    if (!v->cfg.predict_pitch) return fail(nullptr, DSD_EINVAL, "%s: the model has no pitch predictor (predict_pitch = 0)", who);
    if (!sample || !base_pitch || !pitch_pred) return fail(nullptr, DSD_EINVAL, "%s: NULL sample, base_pitch or pitch_pred", who);
    if (int rc = check_sizes(who, B, -1, -1, -1, T)) return rc;
    if (int rc = check_lengths(v, who, B, T)) return rc;
    StagePostP p;
    memset(&p, 0, sizeof(p));
    p.sample = sample; p.base = base_pitch; p.out[0] = pitch_pred;
    p.F = 1; p.T = T; p.M = v->cfg.pitch_repeat_bins;
    p.lo[0] = v->cfg.pitd_clip_min; p.hi[0] = v->cfg.pitd_clip_max; p.clamp[0] = 1;
    HIP_OK(nullptr, hipSetDevice(v->device));
    LAUNCH_OK(who, launch_stage_post(p, B, (hipStream_t)stream), "the post kernel");
    return DSD_OK;
}

int dsd_variance_post(dsd_variance* v, const float* sample, int32_t B, int32_t T, float* const* curves_out, void* stream) {
    const char* who = "dsd_variance_post";
    if (!v) return fail(nullptr, DSD_EINVAL, "%s: NULL object", who);
    if (!v->cfg.variances) return fail(nullptr, DSD_EINVAL, "%s: the model predicts no variance (variances = 0)", who);
    if (!sample || !curves_out) return fail(nullptr, DSD_EINVAL, "%s: NULL sample or curves_out", who);
    for (int i = 0; i < v->n_var; ++i)
        if (!curves_out[i]) return fail(nullptr, DSD_EINVAL, "%s: NULL curves_out[%d] (%s)", who, i, kVarianceNames[v->var_slot[i]]);
    if (int rc = check_sizes(who, B, -1, -1, -1, T)) return rc;
    if ((int64_t)B * T * v->n_var > INT32_MAX) return fail(nullptr, DSD_EINVAL, "%s: B * V * T exceeds 2^31 - 1", who);
    if (int rc = check_lengths(v, who, B, T)) return rc;
    StagePostP p;
    memset(&p, 0, sizeof(p));
    p.sample = sample; p.base = nullptr;
    p.F = v->n_var; p.T = T; p.M = v->cfg.var_repeat_bins;
    for (int i = 0; i < v->n_var; ++i) {
        const int s = v->var_slot[i];
        p.out[i] = curves_out[i];
        p.lo[i] = v->cfg.var_clamp_min[s]; p.hi[i] = v->cfg.var_clamp_max[s]; p.clamp[i] = !v->cfg.var_no_clamp[s];
    }
    HIP_OK(nullptr, hipSetDevice(v->device));
    LAUNCH_OK(who, launch_stage_post(p, B, (hipStream_t)stream), "the post kernel");
    return DSD_OK;
}

int dsd_variance_set_lengths(dsd_variance* v, const int32_t* lengths, int32_t B, void* stream) {
    const char* who = "dsd_variance_set_lengths";
    if (!v) return fail(nullptr, DSD_EINVAL, "%s: NULL object", who);
    if (lengths) {      // everything dsd_set_lengths would refuse, first: the two denoisers are then set both, or neither
        if (B < 1 || B > kMaxItems) return fail(nullptr, DSD_EINVAL, "%s: B = %d outside [1, %d]", who, B, kMaxItems);
        for (int b = 0; b < B; ++b)
            if (lengths[b] < 0) return fail(nullptr, DSD_EINVAL, "%s: lengths[%d] = %d is negative", who, b, lengths[b]);
    }
    if (v->pitch) HANDLE_OK(who, v->pitch, dsd_set_lengths(v->pitch, lengths, B, stream), "the pitch predictor");
    if (v->variances) HANDLE_OK(who, v->variances, dsd_set_lengths(v->variances, lengths, B, stream), "the variance predictor");
    v->ragged = lengths != nullptr;
    if (lengths) v->lengths.assign(lengths, lengths + B);
    else v->lengths.clear();
    return DSD_OK;
}

int dsd_variance_spk_mix(dsd_variance* v, const dsd_spk_mix_args* args, void* stream) {
    const char* who = "dsd_variance_spk_mix";
    if (!v) return fail(nullptr, DSD_EINVAL, "%s: NULL object", who);
    const bool has = v->cfg.use_spk_id && v->ix.spk >= 0;
    return spk_mix_run(who, args, has ? v->tab(v->ix.spk) : nullptr, "the model has no speaker embedding (use_spk_id = 0)",
                       v->cfg.num_spk, v->cfg.hidden_size, v->device, v->spk_ids, stream);
}

}  // extern "C"
