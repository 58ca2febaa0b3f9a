// Stand-alone memory check of the model file reader (diffsinger_amd/csrc/model_file.hip is host code only), under the host
// compiler's address and undefined-behaviour sanitizers.  Takes ONE valid model file (tests/golden/g29_model_v1.dsdm is
// small enough for the quadratic part) and
//   1. opens it and walks every accessor: every name, key and value to its NUL, every config byte, every float of every
//      tensor - a pointer that leaves the file's buffer is a heap overflow the sanitizer reports;
//   2. re-opens every proper prefix of it: each must be refused;
//   3. re-opens copies with each header, directory and table field overwritten by 0, by all-ones and by a value one past
//      its limit, the CRC recomputed (by this file's own bitwise CRC-32) wherever the field lies behind the header, so that
//      the check under test is the one reached.  Such a copy is either refused - a negative code, *out == NULL, a message -
//      or it opens, and then the walk of 1. runs over it: what the reader lets through must be safe to read to the end.
// Not a test of the values (tests/test_modelfile_host.py holds them against the Python writer): what this looks for is a
// read outside the buffer, an integer overflow in the size arithmetic, an allocation sized by a field.  Host only - never
// loaded into Python, needs no GPU:
//
// (one command line)
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude
//       tools/harness/model_harness.cpp -x c++ diffsinger_amd/csrc/model_file.hip -o /tmp/model_harness
//   /tmp/model_harness tests/golden/g29_model_v1.dsdm     # prints one line of counts; exit status 0 = clean
//
// The library proper takes dsd::fail and dsd_last_error from api.hip; this program brings its own.
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include <string>
#include <vector>

#include "dsdenoise.h"

struct dsd_handle;
static std::string g_error;
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
}  // namespace dsd
extern "C" const char* dsd_last_error(const dsd_handle*) { return g_error.c_str(); }

static int g_bad = 0;
static void bad(const char* what, long long where = -1) {
    fprintf(stderr, "%s (at %lld; last error: %s)\n", what, where, g_error.c_str());
    ++g_bad;
}

typedef std::vector<uint8_t> Bytes;

static uint32_t get32(const Bytes& b, size_t off) {
    uint32_t v;
    memcpy(&v, b.data() + off, 4);
    return v;
}
static uint64_t get64(const Bytes& b, size_t off) {
    uint64_t v;
    memcpy(&v, b.data() + off, 8);
    return v;
}
static void put(Bytes& b, size_t off, int width, uint64_t v) { memcpy(b.data() + off, &v, (size_t)width); }     // little-endian host

// zlib's CRC-32, one bit at a time: shares nothing with the reader's table walk
static uint32_t crc32_bitwise(const uint8_t* p, size_t n) {
    uint32_t c = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; ++i) {
        c ^= p[i];
        for (int k = 0; k < 8; ++k) c = (c & 1u) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
    }
    return c ^ 0xFFFFFFFFu;
}
static void fix_crc(Bytes& b) {
    if (b.size() >= 32) put(b, 24, 4, crc32_bitwise(b.data() + 32, b.size() - 32));
}

static std::string g_tmp;
static int open_bytes(const Bytes& b, dsd_model_file** out) {
    FILE* fp = fopen(g_tmp.c_str(), "wb");
    if (!fp || (b.size() && fwrite(b.data(), 1, b.size(), fp) != b.size()) || fclose(fp) != 0) {
        fprintf(stderr, "cannot write %s\n", g_tmp.c_str());
        exit(2);
    }
    g_error.clear();
    return dsd_model_open(g_tmp.c_str(), out);
}

// every byte the accessors hand out, and their own refusals
static volatile double g_sink = 0.0;
static long long walk(const dsd_model_file* f) {
    long long touched = 0;
    int32_t ns = -1, nm = -1;
    if (dsd_model_count(f, &ns, &nm) != DSD_OK || ns < 0 || nm < 0 || ns > DSD_MODEL_MAX_SECTIONS || nm > DSD_MODEL_MAX_META) {
        bad("dsd_model_count");
        return 0;
    }
    dsd_model_section_info si;
    dsd_model_tensor_info ti;
    const char *key = nullptr, *value = nullptr;
    if (dsd_model_section(f, -1, &si) != DSD_EINVAL || dsd_model_section(f, ns, &si) != DSD_EINVAL || dsd_model_section(f, 0, nullptr) != DSD_EINVAL ||
        dsd_model_tensor(f, ns, 0, &ti) != DSD_EINVAL || dsd_model_config(f, ns, &si, 4) != DSD_EINVAL ||
        dsd_model_meta_at(f, nm, &key, &value) != DSD_EINVAL || dsd_model_meta_at(f, -1, &key, &value) != DSD_EINVAL ||
        dsd_model_find(f, nullptr) != DSD_EINVAL || dsd_model_find(f, "no such section \xff") != DSD_ENOTFOUND ||
        dsd_model_meta(f, "no such key \xff") != nullptr || dsd_model_meta(f, nullptr) != nullptr)
        bad("an accessor took an argument it must refuse");
    for (int32_t i = 0; i < ns; ++i) {
        if (dsd_model_section(f, i, &si) != DSD_OK) {
            bad("dsd_model_section", i);
            continue;
        }
        touched += (long long)strlen(si.name);
        if (dsd_model_find(f, si.name) != i) bad("dsd_model_find does not find a section under its own name", i);
        if (si.config_size < 4 || si.config_size > 4096) {
            bad("config size", i);
            continue;
        }
        std::vector<uint8_t> cfg((size_t)si.config_size);        // exactly sized: one byte more is a heap overflow
        if (dsd_model_config(f, i, cfg.data(), si.config_size) != DSD_OK) bad("dsd_model_config", i);
        if (dsd_model_config(f, i, cfg.data(), si.config_size - 1) != DSD_EINVAL) bad("dsd_model_config took a wrong size", i);
        touched += si.config_size;
        int64_t floats = 0;
        if (dsd_model_tensor(f, i, si.n_tensors, &ti) != DSD_EINVAL || dsd_model_tensor(f, i, -1, &ti) != DSD_EINVAL) bad("tensor index", i);
        for (int32_t j = 0; j < si.n_tensors; ++j) {
            if (dsd_model_tensor(f, i, j, &ti) != DSD_OK) {
                bad("dsd_model_tensor", j);
                continue;
            }
            touched += (long long)strlen(ti.name);
            int64_t prod = 1;
            for (int d = 0; d < ti.ndim; ++d) prod *= ti.shape[d];       // the reader promised this cannot overflow: UBSan checks
            if (ti.ndim < 0 || ti.ndim > 4 || prod != ti.count || ((uintptr_t)ti.data % DSD_MODEL_ALIGN) != 0) bad("tensor geometry", j);
            double s = 0.0;
            for (int64_t e = 0; e < ti.count; ++e) s += ti.data[e];
            g_sink = g_sink + s;
            floats += ti.count;
            touched += 4 * ti.count;
        }
        if (floats != si.total_floats) bad("total_floats", i);
    }
    for (int32_t k = 0; k < nm; ++k) {
        if (dsd_model_meta_at(f, k, &key, &value) != DSD_OK) {
            bad("dsd_model_meta_at", k);
            continue;
        }
        touched += (long long)(strlen(key) + strlen(value));
        if (dsd_model_meta(f, key) != value) bad("dsd_model_meta does not find an entry under its own key", k);
    }
    return touched;
}

struct Field {
    size_t off;
    int width;             // 4 or 8 bytes
    uint64_t past_limit;   // a value one past what the field may hold
    const char* name;
};

int main(int argc, char** argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: %s valid_model_file\n", argv[0]);
        return 2;
    }
    Bytes good;
    {
        FILE* fp = fopen(argv[1], "rb");
        if (!fp) {
            fprintf(stderr, "cannot open %s\n", argv[1]);
            return 2;
        }
        uint8_t chunk[4096];
        size_t n;
        while ((n = fread(chunk, 1, sizeof(chunk), fp)) > 0) good.insert(good.end(), chunk, chunk + n);
        fclose(fp);
    }
    char tmpl[] = "/tmp/model_harness_XXXXXX";
    const int fd = mkstemp(tmpl);
    if (fd < 0) return 2;
    close(fd);
    g_tmp = tmpl;

    // 1. the valid file, through the path given and through a copy; the refusals that need no file
    dsd_model_file* f = nullptr;
    long long bytes_walked = 0;
    if (dsd_model_open(argv[1], &f) != DSD_OK || !f) {
        bad("the valid file does not open");
        unlink(g_tmp.c_str());
        return 1;
    }
    bytes_walked = walk(f);
    dsd_model_close(f);
    dsd_model_close(nullptr);
    if (dsd_model_open(nullptr, &f) != DSD_EINVAL || dsd_model_open(argv[1], nullptr) != DSD_EINVAL) bad("NULL arguments");
    if (dsd_model_open("/no/such/directory/model.dsdm", &f) != DSD_EIO || f) bad("a missing path");
    if (dsd_model_open("/tmp", &f) != DSD_EIO || f) bad("a directory");
    if (dsd_model_count(nullptr, nullptr, nullptr) != DSD_EINVAL) bad("dsd_model_count(NULL)");

    // 2. every proper prefix
    int prefixes = 0;
    for (size_t n = 0; n < good.size(); ++n) {
        Bytes cut(good.begin(), good.begin() + (long)n);
        f = reinterpret_cast<dsd_model_file*>(1);
        const int rc = open_bytes(cut, &f);
        if (rc >= 0 || f != nullptr || g_error.empty()) {
            bad("a prefix opened", (long long)n);
            if (rc == DSD_OK) dsd_model_close(f);
        }
        ++prefixes;
    }

    // 3. every field of the header, the directory and the tables
    const uint64_t size = good.size();
    std::vector<Field> fields = {
        {0, 8, 0, "magic"}, {8, 4, DSD_MODEL_FORMAT_VERSION + 1, "format version"}, {12, 4, DSD_API_VERSION + 1, "api version"},
        {16, 8, size + 1, "file size"}, {24, 4, get32(good, 24) + 1, "crc"}, {28, 4, 1, "header reserved"},
        {32, 4, DSD_MODEL_MAX_SECTIONS + 1, "n_sections"}, {36, 4, DSD_MODEL_MAX_META + 1, "n_meta"},
        {40, 8, size + 1, "section table offset"}, {48, 8, size + 1, "meta table offset"}, {56, 8, 1, "directory reserved"},
    };
    const uint32_t ns = get32(good, 32), nm = get32(good, 36);
    const uint64_t st = get64(good, 40), mt = get64(good, 48);
    for (uint32_t i = 0; i < ns; ++i) {
        const size_t s = (size_t)st + 40u * i;
        fields.push_back({s + 0, 8, size, "section name offset"});
        fields.push_back({s + 8, 8, size - get32(good, s + 32) + 1, "config offset"});
        fields.push_back({s + 16, 8, size + 1, "tensor table offset"});
        fields.push_back({s + 24, 4, DSD_MODEL_MAX_NAME + 1, "section name length"});
        fields.push_back({s + 28, 4, DSD_HNSEP_VR + 1, "kind"});
        fields.push_back({s + 32, 4, get32(good, s + 32) + 1, "config size"});
        fields.push_back({s + 36, 4, DSD_MODEL_MAX_TENSORS + 1, "n_tensors"});
        fields.push_back({(size_t)get64(good, s + 8), 4, get32(good, s + 32) + 1, "stored struct_size"});
        fields.push_back({(size_t)get64(good, s + 8) + 4, 4, DSD_HNSEP_VR + 1, "second config field"});
        const uint32_t nt = get32(good, s + 36);
        const uint64_t tt = get64(good, s + 16);
        for (uint32_t j = 0; j < nt; ++j) {
            const size_t t = (size_t)tt + 64u * j;
            fields.push_back({t + 0, 8, size, "tensor name offset"});
            fields.push_back({t + 8, 8, (size / DSD_MODEL_ALIGN + 1) * DSD_MODEL_ALIGN, "data offset"});
            fields.push_back({t + 8, 8, get64(good, t + 8) + 1, "data offset, unaligned"});
            fields.push_back({t + 16, 8, get64(good, t + 16) + 1, "count"});
            fields.push_back({t + 16, 8, size / 4 + 1, "count past the file"});
            fields.push_back({t + 24, 4, DSD_MODEL_MAX_NAME + 1, "tensor name length"});
            fields.push_back({t + 28, 4, 5, "ndim"});
            for (int d = 0; d < 4; ++d) {
                fields.push_back({t + 32 + 8u * (size_t)d, 8, (uint64_t)1 << 63, "dim"});
                fields.push_back({t + 32 + 8u * (size_t)d, 8, (uint64_t)1 << 62, "dim whose product overflows"});
            }
        }
    }
    for (uint32_t k = 0; k < nm; ++k) {
        const size_t m = (size_t)mt + 32u * k;
        fields.push_back({m + 0, 8, size, "key offset"});
        fields.push_back({m + 8, 8, size, "value offset"});
        fields.push_back({m + 16, 8, size - get64(good, m + 8), "value length"});
        fields.push_back({m + 24, 4, DSD_MODEL_MAX_NAME + 1, "key length"});
        fields.push_back({m + 28, 4, 1, "meta reserved"});
    }
    int refused = 0, opened = 0;
    for (const Field& fd_ : fields) {
        if (fd_.off + (size_t)fd_.width > good.size()) {
            bad("a field of the valid file lies outside it", (long long)fd_.off);
            continue;
        }
        const uint64_t values[3] = {0, ~(uint64_t)0, fd_.past_limit};
        for (uint64_t v : values) {
            Bytes b = good;
            put(b, fd_.off, fd_.width, v);
            if (fd_.off >= 32) fix_crc(b);
            f = reinterpret_cast<dsd_model_file*>(1);
            const int rc = open_bytes(b, &f);
            if (rc == DSD_OK && f) {
                bytes_walked += walk(f);
                dsd_model_close(f);
                ++opened;
            } else if (rc < 0 && f == nullptr && !g_error.empty()) {
                ++refused;
            } else {
                bad(fd_.name, (long long)fd_.off);
            }
        }
    }
    unlink(g_tmp.c_str());
    printf("model_harness: %d prefixes refused, %zu fields x 3 values: %d refused, %d opened and walked, %lld bytes read through the "
           "accessors, %d unexpected results\n", prefixes, fields.size(), refused, opened, bytes_walked, g_bad);
    return g_bad ? 1 : 0;
}
