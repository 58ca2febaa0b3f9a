// libdsdenoise, the model file reader: dsd_model_open / _close / _count / _find / _section / _config / _tensor / _meta_at /
// _meta.  Host code only - no kernel, no HIP call, no HIP header - so the same file also compiles with a plain host C++
// compiler (tools/harness/model_harness.cpp builds it that way, under the sanitizers).  dsd_model_create, which turns a
// section into a handle, is model_api.hip.
//
// The layout (format version 1) is DESIGN.md section 4n; diffsinger_amd/modelfile.py is the writer and the second,
// independent statement of it.  Everything is little-endian and read with memcpy at byte offsets: nothing in the file has
// to be aligned for the reader but the tensor data, which the accessors hand out as const float*.
//
// The one rule of this file: dsd_model_open checks every byte an accessor will ever read, the accessors check nothing but
// their own arguments.  Every sum or product of two file fields is formed only after the check that it cannot overflow
// (in_range() subtracts, it never adds), and the only allocations are the file's own bytes - sized by fstat, not by a
// field - and index arrays whose length was first checked against the bytes their table occupies in the file.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>

#include <algorithm>
#include <exception>
#include <vector>

#include "../../include/dsdenoise.h"

#if defined(__BYTE_ORDER__) && __BYTE_ORDER__ != __ORDER_LITTLE_ENDIAN__
#error "model_file.hip reads little-endian fields with memcpy: a big-endian host needs byte swaps"
#endif

struct dsd_handle;
namespace dsd {
// api.hip: records the message for dsd_last_error(NULL) when h == nullptr and returns `code`
int fail(dsd_handle* h, int code, const char* fmt, ...);
}  // namespace dsd
using dsd::fail;

namespace {

// ------------------------------------------------------------------------------------------
// DESIGN.md section 4n, as offsets
// ------------------------------------------------------------------------------------------
const char kMagic[8] = {'D', 'S', 'D', 'M', 'O', 'D', 'E', 'L'};
enum { HDR_MAGIC = 0, HDR_FORMAT = 8, HDR_API = 12, HDR_SIZE = 16, HDR_CRC = 24, HDR_BYTES = 32 };        // not under the CRC
enum { DIR_NSEC = 32, DIR_NMETA = 36, DIR_SEC_TABLE = 40, DIR_META_TABLE = 48, DIR_END = 64 };             // first bytes under it
enum { SEC_NAME = 0, SEC_CONFIG = 8, SEC_TENSORS = 16, SEC_NAME_LEN = 24, SEC_KIND = 28, SEC_CONFIG_SIZE = 32, SEC_NTENSORS = 36,
       SEC_BYTES = 40 };
enum { TEN_NAME = 0, TEN_DATA = 8, TEN_COUNT = 16, TEN_NAME_LEN = 24, TEN_NDIM = 28, TEN_SHAPE = 32, TEN_BYTES = 64 };
enum { META_KEY = 0, META_VALUE = 8, META_VALUE_LEN = 16, META_KEY_LEN = 24, META_BYTES = 32 };

inline uint32_t rd32(const uint8_t* p) {
    uint32_t v;
    memcpy(&v, p, 4);
    return v;
}
inline uint64_t rd64(const uint8_t* p) {
    uint64_t v;
    memcpy(&v, p, 8);
    return v;
}

// zlib's CRC-32 (reflected polynomial 0xEDB88320, initial value and final xor 0xFFFFFFFF), eight bytes a step
struct CrcTables {
    uint32_t t[8][256];
    CrcTables() {
        for (uint32_t i = 0; i < 256; ++i) {
            uint32_t c = i;
            for (int k = 0; k < 8; ++k) c = (c & 1u) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
            t[0][i] = c;
        }
        for (uint32_t i = 0; i < 256; ++i)
            for (int s = 1; s < 8; ++s) t[s][i] = (t[s - 1][i] >> 8) ^ t[0][t[s - 1][i] & 0xFFu];
    }
};
uint32_t crc32_of(const uint8_t* p, uint64_t n) {
    static const CrcTables T;
    uint32_t c = 0xFFFFFFFFu;
    while (n >= 8) {
        const uint32_t lo = rd32(p) ^ c, hi = rd32(p + 4);
        c = T.t[7][lo & 0xFFu] ^ T.t[6][(lo >> 8) & 0xFFu] ^ T.t[5][(lo >> 16) & 0xFFu] ^ T.t[4][lo >> 24] ^
            T.t[3][hi & 0xFFu] ^ T.t[2][(hi >> 8) & 0xFFu] ^ T.t[1][(hi >> 16) & 0xFFu] ^ T.t[0][hi >> 24];
        p += 8;
        n -= 8;
    }
    for (; n; --n) c = T.t[0][(c ^ *p++) & 0xFFu] ^ (c >> 8);
    return c ^ 0xFFFFFFFFu;
}

struct KindInfo {
    const char* what;
    const char* cfg_name;
    uint32_t cfg_size;
};
// indexed by the DSD_* kind
const KindInfo kKinds[] = {
    {"a WaveNet denoiser", "dsd_config", (uint32_t)sizeof(dsd_config)},
    {"a LYNXNet denoiser", "dsd_config", (uint32_t)sizeof(dsd_config)},
    {"an aux decoder", "dsd_config", (uint32_t)sizeof(dsd_config)},
    {"an acoustic encoder", "dsd_encoder_config", (uint32_t)sizeof(dsd_encoder_config)},
    {"a vocoder", "dsd_vocoder_config", (uint32_t)sizeof(dsd_vocoder_config)},
    {"a token encoder", "dsd_token_encoder_config", (uint32_t)sizeof(dsd_token_encoder_config)},
    {"a mel analysis section", "dsd_mel_config", (uint32_t)sizeof(dsd_mel_config)},
    {"an RMVPE pitch extractor", "dsd_rmvpe_config", (uint32_t)sizeof(dsd_rmvpe_config)},
    {"a harmonic-noise separator", "dsd_hnsep_config", (uint32_t)sizeof(dsd_hnsep_config)},
    {nullptr, nullptr, 0},          // 9 is not assigned
    {"the variance model's tables", "dsd_variance_config", (uint32_t)sizeof(dsd_variance_config)},
    {"the acoustic model's tables", "dsd_acoustic_config", (uint32_t)sizeof(dsd_acoustic_config)},
};
const uint32_t kNumKinds = (uint32_t)(sizeof(kKinds) / sizeof(kKinds[0]));

}  // namespace

struct dsd_model_file {
    uint8_t* buf = nullptr;
    uint64_t size = 0;
    uint32_t n_sections = 0, n_meta = 0;
    uint64_t sec_table = 0, meta_table = 0;
    std::vector<int64_t> total_floats;      // per section
    ~dsd_model_file() { free(buf); }

    const uint8_t* sec(uint32_t i) const { return buf + sec_table + (uint64_t)i * SEC_BYTES; }
    const uint8_t* ten(uint32_t i, uint32_t j) const { return buf + rd64(sec(i) + SEC_TENSORS) + (uint64_t)j * TEN_BYTES; }
    const uint8_t* meta(uint32_t k) const { return buf + meta_table + (uint64_t)k * META_BYTES; }
    const char* str(uint64_t off) const { return reinterpret_cast<const char*>(buf + off); }
};

namespace {

const char* const WHO = "dsd_model_open";

// [off, off + len) lies inside the file; formed without an addition that could wrap
inline bool in_range(const dsd_model_file& f, uint64_t off, uint64_t len) { return off <= f.size && len <= f.size - off; }

// a section name, tensor name or metadata key: 1 .. 255 bytes without a NUL, followed by one.  `what` already names the owner.
int check_name(const dsd_model_file& f, uint64_t off, uint32_t len, const char* what) {
    if (len == 0) return fail(nullptr, DSD_EINVAL, "%s: %s is empty", WHO, what);
    if (len > DSD_MODEL_MAX_NAME) return fail(nullptr, DSD_EINVAL, "%s: %s is longer than %d bytes (%u)", WHO, what, DSD_MODEL_MAX_NAME, len);
    if (!in_range(f, off, (uint64_t)len + 1))
        return fail(nullptr, DSD_EINVAL, "%s: %s (offset %llu, %u bytes) is past the end of the file", WHO, what, (unsigned long long)off, len);
    if (memchr(f.buf + off, 0, len)) return fail(nullptr, DSD_EINVAL, "%s: %s holds a NUL", WHO, what);
    if (f.buf[off + len] != 0) return fail(nullptr, DSD_EINVAL, "%s: %s is not NUL-terminated", WHO, what);
    return DSD_OK;
}

struct NameRef {
    const uint8_t* p;
    uint32_t len;
    uint32_t index;
};
// -> the index of the second of two equal names, or -1.  Sorts: 65536 names must not cost 65536^2 comparisons.
int64_t find_duplicate(std::vector<NameRef>& names) {
    auto less = [](const NameRef& a, const NameRef& b) {
        if (a.len != b.len) return a.len < b.len;
        const int c = memcmp(a.p, b.p, a.len);
        return c != 0 ? c < 0 : a.index < b.index;
    };
    std::sort(names.begin(), names.end(), less);
    for (size_t i = 1; i < names.size(); ++i)
        if (names[i].len == names[i - 1].len && memcmp(names[i].p, names[i - 1].p, names[i].len) == 0) return names[i].index;
    return -1;
}

int check_tensor(const dsd_model_file& f, uint32_t i, const char* sname, uint32_t j, const uint8_t* t, int64_t* count_out) {
    char what[96];
    snprintf(what, sizeof(what), "section %u tensor %u: the name", i, j);
    const uint64_t name_off = rd64(t + TEN_NAME);
    const uint32_t name_len = rd32(t + TEN_NAME_LEN);
    if (int rc = check_name(f, name_off, name_len, what)) return rc;
    const char* name = f.str(name_off);
    const uint32_t ndim = rd32(t + TEN_NDIM);
    if (ndim > 4) return fail(nullptr, DSD_EINVAL, "%s: section \"%s\" tensor \"%s\": ndim %u > 4", WHO, sname, name, ndim);
    // the product of the dims: 0 if any is 0, else checked against 2^63 - 1 factor by factor
    uint64_t prod = 1;
    bool zero = false;
    for (uint32_t d = 0; d < ndim; ++d) {
        const int64_t v = (int64_t)rd64(t + TEN_SHAPE + 8 * d);
        if (v < 0) return fail(nullptr, DSD_EINVAL, "%s: section \"%s\" tensor \"%s\": negative dim %lld at axis %u", WHO, sname, name, (long long)v, d);
        if (v == 0) zero = true;
    }
    if (zero) prod = 0;
    else
        for (uint32_t d = 0; d < ndim; ++d) {
            const uint64_t v = rd64(t + TEN_SHAPE + 8 * d);
            if (prod > (uint64_t)INT64_MAX / v)
                return fail(nullptr, DSD_EINVAL, "%s: section \"%s\" tensor \"%s\": the shape product overflows 64 bits", WHO, sname, name);
            prod *= v;
        }
    const uint64_t count = rd64(t + TEN_COUNT);
    if (prod != count)
        return fail(nullptr, DSD_EINVAL, "%s: section \"%s\" tensor \"%s\": the shape product %llu differs from the stored count %llu", WHO,
                    sname, name, (unsigned long long)prod, (unsigned long long)count);
    const uint64_t data = rd64(t + TEN_DATA);
    if (data % DSD_MODEL_ALIGN != 0)
        return fail(nullptr, DSD_EINVAL, "%s: section \"%s\" tensor \"%s\": data offset %llu is not %d-byte aligned", WHO, sname, name,
                    (unsigned long long)data, DSD_MODEL_ALIGN);
    // count * 4 bytes from `data`: compare the count with the floats that are left, so that nothing is multiplied
    if (data > f.size || count > (f.size - data) / 4)
        return fail(nullptr, DSD_EINVAL, "%s: section \"%s\" tensor \"%s\": data (offset %llu, %llu floats) is past the end of the file", WHO,
                    sname, name, (unsigned long long)data, (unsigned long long)count);
    *count_out = (int64_t)count;        // <= size / 4
    return DSD_OK;
}

int check_section(dsd_model_file& f, uint32_t i) {
    const uint8_t* s = f.sec(i);
    char what[64];
    snprintf(what, sizeof(what), "section %u: the name", i);
    const uint64_t name_off = rd64(s + SEC_NAME);
    if (int rc = check_name(f, name_off, rd32(s + SEC_NAME_LEN), what)) return rc;
    const char* sname = f.str(name_off);
    const uint32_t kind = rd32(s + SEC_KIND);
    if (kind >= kNumKinds || !kKinds[kind].what)
        return fail(nullptr, DSD_EINVAL, "%s: section \"%s\": unknown kind %u (the DSD_* kinds are 0 .. %d, %d and %d)", WHO, sname, kind,
                    (int)DSD_HNSEP_VR, (int)DSD_VARIANCE_TABLES, (int)DSD_ACOUSTIC_TABLES);
    const KindInfo& K = kKinds[kind];
    const uint32_t cfg_size = rd32(s + SEC_CONFIG_SIZE);
    if (cfg_size != K.cfg_size)
        return fail(nullptr, DSD_EINVAL, "%s: section \"%s\" (%s): config size %u is not sizeof(%s) = %u", WHO, sname, K.what, cfg_size, K.cfg_name, K.cfg_size);
    const uint64_t cfg_off = rd64(s + SEC_CONFIG);
    if (!in_range(f, cfg_off, cfg_size))
        return fail(nullptr, DSD_EINVAL, "%s: section \"%s\": the config (offset %llu, %u bytes) is past the end of the file", WHO, sname,
                    (unsigned long long)cfg_off, cfg_size);
    // every config struct starts with int32 struct_size; a dsd_config goes on with int32 backbone
    const int32_t struct_size = (int32_t)rd32(f.buf + cfg_off);
    if (struct_size < 0 || (uint32_t)struct_size != cfg_size)
        return fail(nullptr, DSD_EINVAL, "%s: section \"%s\": the stored struct_size %d disagrees with the config size %u", WHO, sname, struct_size, cfg_size);
    if (kind <= (uint32_t)DSD_AUX_CONVNEXT && rd32(f.buf + cfg_off + 4) != kind)
        return fail(nullptr, DSD_EINVAL, "%s: section \"%s\" is of kind %u, its dsd_config says backbone %d", WHO, sname, kind, (int)rd32(f.buf + cfg_off + 4));
    const uint32_t n_tensors = rd32(s + SEC_NTENSORS);
    if (n_tensors > DSD_MODEL_MAX_TENSORS)
        return fail(nullptr, DSD_EINVAL, "%s: section \"%s\": %u tensors are over the limit of %d", WHO, sname, n_tensors, DSD_MODEL_MAX_TENSORS);
    if (kind == (uint32_t)DSD_MEL_ANALYSIS && n_tensors != 0)
        return fail(nullptr, DSD_EINVAL, "%s: section \"%s\": a mel analysis section has no tensors (%u stored)", WHO, sname, n_tensors);
    const uint64_t table = rd64(s + SEC_TENSORS);
    if (!in_range(f, table, (uint64_t)n_tensors * TEN_BYTES))        // <= 65536 * 64: no overflow
        return fail(nullptr, DSD_EINVAL, "%s: section \"%s\": the tensor table (offset %llu, %u entries) is past the end of the file", WHO, sname,
                    (unsigned long long)table, n_tensors);
    std::vector<NameRef> names;
    names.reserve(n_tensors);           // n_tensors * 64 bytes of table are in the file
    int64_t total = 0;
    for (uint32_t j = 0; j < n_tensors; ++j) {
        const uint8_t* t = f.buf + table + (uint64_t)j * TEN_BYTES;
        int64_t count = 0;
        if (int rc = check_tensor(f, i, sname, j, t, &count)) return rc;
        if (count > INT64_MAX - total) return fail(nullptr, DSD_EINVAL, "%s: section \"%s\": the tensors' counts overflow 64 bits", WHO, sname);
        total += count;
        names.push_back({f.buf + rd64(t + TEN_NAME), rd32(t + TEN_NAME_LEN), j});
    }
    const int64_t dup = find_duplicate(names);
    if (dup >= 0)
        return fail(nullptr, DSD_EINVAL, "%s: section \"%s\": two tensors are called \"%s\"", WHO, sname, f.str(rd64(f.ten(i, (uint32_t)dup) + TEN_NAME)));
    f.total_floats[i] = total;
    return DSD_OK;
}

int check_meta(const dsd_model_file& f, uint32_t k) {
    const uint8_t* m = f.meta(k);
    char what[64];
    snprintf(what, sizeof(what), "metadata entry %u: the key", k);
    const uint64_t key_off = rd64(m + META_KEY);
    if (int rc = check_name(f, key_off, rd32(m + META_KEY_LEN), what)) return rc;
    const char* key = f.str(key_off);
    const uint64_t off = rd64(m + META_VALUE), len = rd64(m + META_VALUE_LEN);
    // len bytes and the NUL behind them: len < the bytes that are left
    if (off > f.size || len >= f.size - off)
        return fail(nullptr, DSD_EINVAL, "%s: metadata \"%s\": the value (offset %llu, %llu bytes) is past the end of the file", WHO, key,
                    (unsigned long long)off, (unsigned long long)len);
    if (len && memchr(f.buf + off, 0, len)) return fail(nullptr, DSD_EINVAL, "%s: metadata \"%s\": the value holds a NUL", WHO, key);
    if (f.buf[off + len] != 0) return fail(nullptr, DSD_EINVAL, "%s: metadata \"%s\": the value is not NUL-terminated", WHO, key);
    return DSD_OK;
}

// everything behind the file's bytes: f.buf / f.size are set
int validate(dsd_model_file& f) {
    if (f.size < DIR_END) return fail(nullptr, DSD_EINVAL, "%s: %llu bytes are fewer than the %d of a header", WHO, (unsigned long long)f.size, (int)DIR_END);
    if (memcmp(f.buf + HDR_MAGIC, kMagic, sizeof(kMagic)) != 0) return fail(nullptr, DSD_EINVAL, "%s: bad magic (not a model file)", WHO);
    const uint32_t version = rd32(f.buf + HDR_FORMAT);
    if (version != DSD_MODEL_FORMAT_VERSION)
        return fail(nullptr, DSD_EINVAL, "%s: format version %u is unknown (this library reads version %d)", WHO, version, DSD_MODEL_FORMAT_VERSION);
    const uint64_t recorded = rd64(f.buf + HDR_SIZE);
    if (recorded != f.size)
        return fail(nullptr, DSD_EINVAL, "%s: the header records %llu bytes, the file has %llu", WHO, (unsigned long long)recorded, (unsigned long long)f.size);
    const uint32_t stored = rd32(f.buf + HDR_CRC), computed = crc32_of(f.buf + HDR_BYTES, f.size - HDR_BYTES);
    if (stored != computed) return fail(nullptr, DSD_EINVAL, "%s: CRC mismatch (stored %08x, computed %08x)", WHO, stored, computed);

    f.n_sections = rd32(f.buf + DIR_NSEC);
    f.n_meta = rd32(f.buf + DIR_NMETA);
    if (f.n_sections > DSD_MODEL_MAX_SECTIONS)
        return fail(nullptr, DSD_EINVAL, "%s: %u sections are over the limit of %d", WHO, f.n_sections, DSD_MODEL_MAX_SECTIONS);
    if (f.n_meta > DSD_MODEL_MAX_META)
        return fail(nullptr, DSD_EINVAL, "%s: %u metadata entries are over the limit of %d", WHO, f.n_meta, DSD_MODEL_MAX_META);
    f.sec_table = rd64(f.buf + DIR_SEC_TABLE);
    f.meta_table = rd64(f.buf + DIR_META_TABLE);
    if (!in_range(f, f.sec_table, (uint64_t)f.n_sections * SEC_BYTES))
        return fail(nullptr, DSD_EINVAL, "%s: the section table (offset %llu, %u entries) is past the end of the file", WHO,
                    (unsigned long long)f.sec_table, f.n_sections);
    if (!in_range(f, f.meta_table, (uint64_t)f.n_meta * META_BYTES))
        return fail(nullptr, DSD_EINVAL, "%s: the metadata table (offset %llu, %u entries) is past the end of the file", WHO,
                    (unsigned long long)f.meta_table, f.n_meta);

    f.total_floats.assign(f.n_sections, 0);
    std::vector<NameRef> names;
    for (uint32_t i = 0; i < f.n_sections; ++i) {
        if (int rc = check_section(f, i)) return rc;
        names.push_back({f.buf + rd64(f.sec(i) + SEC_NAME), rd32(f.sec(i) + SEC_NAME_LEN), i});
    }
    int64_t dup = find_duplicate(names);
    if (dup >= 0) return fail(nullptr, DSD_EINVAL, "%s: two sections are called \"%s\"", WHO, f.str(rd64(f.sec((uint32_t)dup) + SEC_NAME)));
    names.clear();
    names.reserve(f.n_meta);
    for (uint32_t k = 0; k < f.n_meta; ++k) {
        if (int rc = check_meta(f, k)) return rc;
        names.push_back({f.buf + rd64(f.meta(k) + META_KEY), rd32(f.meta(k) + META_KEY_LEN), k});
    }
    dup = find_duplicate(names);
    if (dup >= 0) return fail(nullptr, DSD_EINVAL, "%s: two metadata entries have the key \"%s\"", WHO, f.str(rd64(f.meta((uint32_t)dup) + META_KEY)));
    return DSD_OK;
}

int read_file(const char* path, dsd_model_file& f) {
    FILE* fp = fopen(path, "rb");
    if (!fp) return fail(nullptr, DSD_EIO, "%s: cannot open %s", WHO, path);
    struct stat st;
    if (fstat(fileno(fp), &st) != 0 || !S_ISREG(st.st_mode) || st.st_size < 0) {
        fclose(fp);
        return fail(nullptr, DSD_EIO, "%s: %s is not a regular file", WHO, path);
    }
    f.size = (uint64_t)st.st_size;
    // the buffer is sized by the file system's answer, not by a field of the file; aligned so that 64-byte aligned
    // offsets are 64-byte aligned pointers
    const uint64_t rounded = (f.size / DSD_MODEL_ALIGN + 1) * DSD_MODEL_ALIGN;
    void* mem = nullptr;
    if (rounded > (uint64_t)SIZE_MAX || posix_memalign(&mem, DSD_MODEL_ALIGN, (size_t)rounded) != 0 || !mem) {
        fclose(fp);
        return fail(nullptr, DSD_ENOMEM, "%s: no host memory for the %llu bytes of %s", WHO, (unsigned long long)f.size, path);
    }
    f.buf = static_cast<uint8_t*>(mem);
    uint64_t got = 0;
    while (got < f.size) {
        const size_t n = fread(f.buf + got, 1, (size_t)std::min<uint64_t>(f.size - got, (uint64_t)1 << 30), fp);
        if (n == 0) break;
        got += n;
    }
    const bool more = got == f.size && fgetc(fp) != EOF;        // the file grew while it was read
    fclose(fp);
    if (got != f.size || more) return fail(nullptr, DSD_EIO, "%s: %s could not be read to its end (%llu of %llu bytes)", WHO, path,
                                           (unsigned long long)got, (unsigned long long)f.size);
    memset(f.buf + f.size, 0, (size_t)(rounded - f.size));
    return DSD_OK;
}

}  // namespace

extern "C" {

int dsd_model_open(const char* path, dsd_model_file** out) {
    if (out) *out = nullptr;
    if (!path || !out) return fail(nullptr, DSD_EINVAL, "%s: NULL argument", WHO);
    dsd_model_file* f = nullptr;
    try {
        f = new dsd_model_file();
        int rc = read_file(path, *f);
        if (rc == DSD_OK) rc = validate(*f);
        if (rc != DSD_OK) {
            delete f;
            return rc;
        }
    } catch (const std::exception&) {
        delete f;
        return fail(nullptr, DSD_ENOMEM, "%s: out of host memory", WHO);
    }
    *out = f;
    return DSD_OK;
}

void dsd_model_close(dsd_model_file* f) { delete f; }

int dsd_model_count(const dsd_model_file* f, int32_t* n_sections, int32_t* n_meta) {
    if (!f) return fail(nullptr, DSD_EINVAL, "dsd_model_count: NULL file");
    if (n_sections) *n_sections = (int32_t)f->n_sections;
    if (n_meta) *n_meta = (int32_t)f->n_meta;
    return DSD_OK;
}

int dsd_model_find(const dsd_model_file* f, const char* section_name) {
    if (!f || !section_name) return fail(nullptr, DSD_EINVAL, "dsd_model_find: NULL argument");
    const size_t len = strlen(section_name);
    for (uint32_t i = 0; i < f->n_sections; ++i)
        if (rd32(f->sec(i) + SEC_NAME_LEN) == len && memcmp(f->str(rd64(f->sec(i) + SEC_NAME)), section_name, len) == 0) return (int)i;
    return fail(nullptr, DSD_ENOTFOUND, "dsd_model_find: no section is called \"%s\"", section_name);
}

int dsd_model_section(const dsd_model_file* f, int32_t i, dsd_model_section_info* out) {
    if (!f || !out) return fail(nullptr, DSD_EINVAL, "dsd_model_section: NULL argument");
    if (i < 0 || (uint32_t)i >= f->n_sections) return fail(nullptr, DSD_EINVAL, "dsd_model_section: section %d out of range [0, %u)", i, f->n_sections);
    const uint8_t* s = f->sec((uint32_t)i);
    out->name = f->str(rd64(s + SEC_NAME));
    out->kind = (int32_t)rd32(s + SEC_KIND);
    out->config_size = (int32_t)rd32(s + SEC_CONFIG_SIZE);
    out->n_tensors = (int32_t)rd32(s + SEC_NTENSORS);
    out->total_floats = f->total_floats[(size_t)i];
    return DSD_OK;
}

int dsd_model_config(const dsd_model_file* f, int32_t i, void* cfg_out, int32_t cfg_size) {
    if (!f || !cfg_out) return fail(nullptr, DSD_EINVAL, "dsd_model_config: NULL argument");
    if (i < 0 || (uint32_t)i >= f->n_sections) return fail(nullptr, DSD_EINVAL, "dsd_model_config: section %d out of range [0, %u)", i, f->n_sections);
    const uint8_t* s = f->sec((uint32_t)i);
    const uint32_t kind = rd32(s + SEC_KIND), size = rd32(s + SEC_CONFIG_SIZE);
    if (cfg_size < 0 || (uint32_t)cfg_size != size)
        return fail(nullptr, DSD_EINVAL, "dsd_model_config: section \"%s\" is %s, its config is a %s of %u bytes, not %d", f->str(rd64(s + SEC_NAME)),
                    kKinds[kind].what, kKinds[kind].cfg_name, size, cfg_size);
    memcpy(cfg_out, f->buf + rd64(s + SEC_CONFIG), size);
    return DSD_OK;
}

int dsd_model_tensor(const dsd_model_file* f, int32_t i, int32_t j, dsd_model_tensor_info* out) {
    if (!f || !out) return fail(nullptr, DSD_EINVAL, "dsd_model_tensor: NULL argument");
    if (i < 0 || (uint32_t)i >= f->n_sections) return fail(nullptr, DSD_EINVAL, "dsd_model_tensor: section %d out of range [0, %u)", i, f->n_sections);
    const uint32_t n = rd32(f->sec((uint32_t)i) + SEC_NTENSORS);
    if (j < 0 || (uint32_t)j >= n) return fail(nullptr, DSD_EINVAL, "dsd_model_tensor: tensor %d of section %d out of range [0, %u)", j, i, n);
    const uint8_t* t = f->ten((uint32_t)i, (uint32_t)j);
    out->name = f->str(rd64(t + TEN_NAME));
    out->ndim = (int32_t)rd32(t + TEN_NDIM);
    for (int d = 0; d < 4; ++d) out->shape[d] = d < out->ndim ? (int64_t)rd64(t + TEN_SHAPE + 8 * d) : 0;
    out->count = (int64_t)rd64(t + TEN_COUNT);
    out->data = reinterpret_cast<const float*>(f->buf + rd64(t + TEN_DATA));
    return DSD_OK;
}

int dsd_model_meta_at(const dsd_model_file* f, int32_t k, const char** key, const char** value) {
    if (!f || !key || !value) return fail(nullptr, DSD_EINVAL, "dsd_model_meta_at: NULL argument");
    if (k < 0 || (uint32_t)k >= f->n_meta) return fail(nullptr, DSD_EINVAL, "dsd_model_meta_at: entry %d out of range [0, %u)", k, f->n_meta);
    *key = f->str(rd64(f->meta((uint32_t)k) + META_KEY));
    *value = f->str(rd64(f->meta((uint32_t)k) + META_VALUE));
    return DSD_OK;
}

const char* dsd_model_meta(const dsd_model_file* f, const char* key) {
    if (!f || !key) return nullptr;
    const size_t len = strlen(key);
    for (uint32_t k = 0; k < f->n_meta; ++k) {
        const uint8_t* m = f->meta(k);
        if (rd32(m + META_KEY_LEN) == len && memcmp(f->str(rd64(m + META_KEY)), key, len) == 0) return f->str(rd64(m + META_VALUE));
    }
    return nullptr;
}

}  // extern "C"
