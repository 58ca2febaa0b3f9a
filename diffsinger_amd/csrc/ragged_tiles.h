// Ragged batches, the host's one description of them: B items padded to T frames, item b holding lengths[b] valid ones, and the
// (item, frame tile) pairs that therefore exist.  One builder (build_ragged) makes the lengths and valid-tile lists of a batch
// at every rate it runs at, one view (RaggedGrid) hands a batch at one rate to the launchers, one filler (fill_tiles) sets
// every launcher's tile fields from it.  A null grid is a dense batch everywhere.  Plain C++ without a HIP header, so a host
// compiler takes it (tools/harness/ragged_harness.cpp); the owner of the device block is RaggedOwner in api_host.h.
#pragma once
#include <stddef.h>

#include <algorithm>
#include <vector>

namespace dsd {

// the tile widths a list can be built at: the GEMM / layer kernels' 16, 32 and 64 frames, tconv.hip's 256
constexpr int kRagWidths[4] = {16, 32, 64, 256};
inline int rag_k(int bn) { return bn == 16 ? 0 : bn == 32 ? 1 : bn == 64 ? 2 : 3; }
enum : unsigned { RAG_W16 = 1, RAG_W32 = 2, RAG_W64 = 4, RAG_W256 = 8 };

// A ragged batch at one rate, as the launchers take it (nullptr = dense).  Whoever builds it sets the two policies.
struct RaggedGrid {
    int B = 0, T = 0;                   // T: the padded length at this rate
    long valid = 0;                     // the sum of the lengths (a long: B items of up to 2^28 samples)
    int count[4] = {};                  // tiles with valid frames at kRagWidths[k], whether a list was asked for or not
    size_t lens_at = 0, list_at[4] = {};    // where the [B] lengths and the lists lie in the block (a list not asked for: kNoList)
    const int* lens = nullptr;          // device: the lengths ...
    const int* list[4] = {};            // ... and the valid-tile lists (nullptr: not built)
    const int* lens_host = nullptr;     // host mirrors
    const int* list_host[4] = {};
    // Tile-width policy: make_gemm takes 64-frame tiles from 512 workgroups up.  The denoisers count them over the PADDED batch
    // (false: a ragged batch keeps the tile width of its dense shape, as the planner's measurements were taken); the vocoder
    // counts the valid tiles (true: the width B lone calls of similar length would take)
    bool nb_by_valid_tiles = false;
    // Input-masking policy: the denoisers give the lengths only to k-tap GEMMs (false: only a convolution along time can carry
    // padded frames into valid ones, and their 1x1s read activations whose padding nobody zeroed); the vocoder gives them to
    // every GEMM (true), which includes a transposed conv whose phase-row GEMM has one tap (kernel == rate)
    bool mask_every_gemm = false;
    static constexpr size_t kNoList = ~(size_t)0;
    void point(const int* host, const int* dev) {      // the block's host copy and its device copy (nullptr: not uploaded yet)
        lens_host = host + lens_at;
        lens = dev ? dev + lens_at : nullptr;
        for (int k = 0; k < 4; ++k) {
            list_host[k] = list_at[k] != kNoList ? host + list_at[k] : nullptr;
            list[k] = dev && list_host[k] ? dev + list_at[k] : nullptr;
        }
    }
};

// `out` = per rate r (lengths and T scaled by mult[r]): the B lengths, then for every width of the `widths` mask the list of
// b * ceil(T_r / BN) + ft for every ft with ft * BN < len_b - ITEM-MAJOR AND ASCENDING, so tiles [t0, t0 + nt) of the batch's
// (item, frame tile) order are the slice list + t0 of nt entries (run_wavenet's segments rely on it), and the first half of
// 32-frame tile n has a 16-frame index that a prefix walk over the lengths finds (rag_map16).  A zero-length item adds nothing;
// an all-empty batch gives empty lists.  `grids` = per rate where its parts lie, the count of valid tiles at every width and
// the sum of the lengths (host-only facts: they stay out of the block), pointing into `out`.  Returns the size of the same
// block with every item T long: what an owner reserves, so that other lengths of the same (B, T) never move the block.
inline size_t build_ragged(const int* lengths, int B, int T, unsigned widths, const std::vector<long>& mult,
                           std::vector<int>& out, std::vector<RaggedGrid>& grids) {
    out.clear();
    grids.assign(mult.size(), RaggedGrid());
    size_t dense = 0;
    for (size_t r = 0; r < mult.size(); ++r) {
        RaggedGrid& g = grids[r];
        g.B = B;
        g.T = (int)(T * mult[r]);
        g.lens_at = out.size();
        for (int b = 0; b < B; ++b) {
            out.push_back((int)(lengths[b] * mult[r]));
            g.valid += lengths[b] * mult[r];
        }
        dense += B;
        for (int k = 0; k < 4; ++k) {
            const int BN = kRagWidths[k], tiles = (g.T + BN - 1) / BN;
            const bool listed = widths >> k & 1;
            g.list_at[k] = listed ? out.size() : RaggedGrid::kNoList;
            for (int b = 0; b < B; ++b) {
                const int n = (int)((lengths[b] * mult[r] + BN - 1) / BN);
                g.count[k] += n;
                for (int ft = 0; listed && ft < n; ++ft) out.push_back(b * tiles + ft);
            }
            if (listed) dense += (size_t)B * tiles;
        }
    }
    for (RaggedGrid& g : grids) g.point(out.data(), nullptr);
    return dense;
}

// valid frame tiles of `bn` frames (16 / 32 / 64 / 256) in the batch
inline long tiles_at(const RaggedGrid* g, int B, int T, int bn) {
    return g ? (long)g->count[rag_k(bn)] : (long)B * ((T + bn - 1) / bn);
}
inline double valid_frames(const RaggedGrid* g, int B, int T) { return g ? (double)g->valid : (double)B * T; }
// valid frames in tiles [t0, t0 + nt) of the (item, frame tile) order at width bn (ragged: of the valid-tile list)
inline double tile_frames(const RaggedGrid* g, int T, int bn, int t0, int nt) {
    const int tpb = (T + bn - 1) / bn;
    double fr = 0;
    for (int i = t0; i < t0 + nt; ++i) {
        const int e = g ? g->list_host[rag_k(bn)][i] : i % tpb, b = e / tpb;
        fr += std::min(bn, (g ? g->lens_host[b] : T) - (e - b * tpb) * bn);
    }
    return fr;
}
// index in the 16-frame tile order of the first 16-frame tile of 32-frame tile n (of the dense order / the valid-tile lists)
inline long rag_map16(const RaggedGrid* g, int T, long n) {
    if (!g) {
        const long tpb32 = (T + 31) / 32, tpb16 = (T + 15) / 16;
        return (n / tpb32) * tpb16 + 2 * (n % tpb32);
    }
    long n32 = 0, n16 = 0;
    for (int b = 0; b < g->B; ++b) {
        const long t32 = (g->lens_host[b] + 31) / 32, t16 = (g->lens_host[b] + 15) / 16;
        if (n < n32 + t32) return n16 + 2 * (n - n32);
        n32 += t32; n16 += t16;
    }
    return n16;
}

// The tile fields of a launcher's parameter block (zeroed by the caller) for a launch on BN-frame tiles: frame tiles per item
// and its reciprocal; ragged also the lengths and the valid-tile list where the struct has the field.  Returns the launch's tile
// count.  (TConvP calls its tiles-per-item `tiles` and has no reciprocal; WnEdgeP and LxLayerP take no lengths.)
template <typename P> auto rag_tpb(P& p, int) -> decltype((p.tiles_per_b)) { return p.tiles_per_b; }
template <typename P> auto rag_tpb(P& p, long) -> decltype((p.tiles)) { return p.tiles; }
template <typename P> auto rag_set_inv(P& p, int) -> decltype((void)p.inv_tiles_per_b) { p.inv_tiles_per_b = 1.0f / (float)rag_tpb(p, 0); }
template <typename P> void rag_set_inv(P&, long) {}
template <typename P> auto rag_set_lens(P& p, const int* lens, int) -> decltype((void)p.lens) { p.lens = lens; }
template <typename P> void rag_set_lens(P&, const int*, long) {}
template <typename P>
long fill_tiles(P& p, const RaggedGrid* g, int B, int T, int BN) {
    rag_tpb(p, 0) = (T + BN - 1) / BN;
    rag_set_inv(p, 0);
    if (!g) return (long)B * rag_tpb(p, 0);
    rag_set_lens(p, g->lens, 0);
    p.cgmap = g->list[rag_k(BN)];
    p.ncg = g->count[rag_k(BN)];
    return p.ncg;
}

}  // namespace dsd
