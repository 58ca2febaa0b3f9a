// Stand-alone check of the ragged-batch builder and the helpers over its output (diffsinger_amd/csrc/ragged_tiles.h is plain
// C++): build_ragged against a brute-force enumeration over (item, frame tile) at the denoisers' rates {1} and the vocoder's
// {1, 8, 64, 512}, for T on, below and above every tile width, lengths on, one below and one above every boundary, a one-frame
// item, a zero-length item in first, middle and last position, an all-empty batch, B = 1 and B = 9 - under the host compiler's
// address and undefined-behaviour sanitizers, so a list entry written or read outside the block is reported.  Also: the lists
// ascend item-major, count[k] is the list's length wherever a list is built, rag_map16 agrees with the prefix walk it replaced
// and with the two lists, tile_frames with a count frame by frame, fill_tiles with the block.  Host only - never loaded into
// Python, needs no GPU:
//
// (one command line)
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Idiffsinger_amd/csrc
//       tools/harness/ragged_harness.cpp -o /tmp/ragged_harness
//   /tmp/ragged_harness             # prints the number of batches and comparisons; exit status 0 = clean
#include <stdio.h>
#include <stdlib.h>

#include <set>
#include <vector>

#include "ragged_tiles.h"

using namespace dsd;

static long g_checks = 0;
#define CHECK(cond)                                                                        \
    do {                                                                                   \
        ++g_checks;                                                                        \
        if (!(cond)) {                                                                     \
            fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond);       \
            exit(1);                                                                       \
        }                                                                                  \
    } while (0)

// a launcher's parameter block with every tile field, one without lengths and reciprocal, and tconv.hip's naming
struct FullP { int tiles_per_b; float inv_tiles_per_b; const int* lens; const int* cgmap; int ncg; };
struct BareP { int tiles_per_b; const int* cgmap; int ncg; };
struct TilesP { int tiles; const int* lens; const int* cgmap; int ncg; };

// the prefix walk of the planner as it stood before rag_map16
static long map16_walk(const std::vector<int>& lens, long n) {
    long n32 = 0, n16 = 0;
    for (int v : lens) {
        const long t32 = (v + 31) / 32, t16 = (v + 15) / 16;
        if (n < n32 + t32) return n16 + 2 * (n - n32);
        n32 += t32; n16 += t16;
    }
    return n16;
}

static void check_batch(const std::vector<int>& lengths, int T, unsigned widths, const std::vector<long>& mult) {
    const int B = (int)lengths.size();
    std::vector<int> out;
    std::vector<RaggedGrid> grids;
    const size_t dense = build_ragged(lengths.data(), B, T, widths, mult, out, grids);
    CHECK(grids.size() == mult.size() && out.size() <= dense);
    size_t at = 0;          // the parts follow each other in the block in the documented order
    for (size_t r = 0; r < mult.size(); ++r) {
        RaggedGrid g = grids[r];
        CHECK(g.B == B && g.T == T * mult[r] && g.lens_at == at && g.lens_host == out.data() + at && !g.lens);
        g.point(out.data(), out.data());        // (the "device" copy is the host's here)
        long sum = 0;
        std::vector<int> lens(B);
        for (int b = 0; b < B; ++b) {
            lens[b] = out[at++];
            CHECK(lens[b] == lengths[b] * mult[r]);
            sum += lens[b];
        }
        CHECK(g.valid == sum && g.lens == g.lens_host);
        for (int k = 0; k < 4; ++k) {
            const int BN = kRagWidths[k], tiles = (g.T + BN - 1) / BN;
            CHECK(rag_k(BN) == k);
            std::vector<int> want;          // brute force over (b, ft)
            for (int b = 0; b < B; ++b)
                for (int ft = 0; ft < tiles; ++ft)
                    if ((long)ft * BN < lens[b]) want.push_back(b * tiles + ft);
            CHECK(g.count[k] == (int)want.size());
            CHECK(tiles_at(&g, B, g.T, BN) == (long)want.size() && tiles_at(nullptr, B, g.T, BN) == (long)B * tiles);
            if (!(widths >> k & 1)) {
                CHECK(!g.list[k] && !g.list_host[k]);
                continue;
            }
            CHECK(g.list_at[k] == at && g.list[k] == out.data() + at && g.list_host[k] == g.list[k]);
            for (size_t i = 0; i < want.size(); ++i) {
                CHECK(out[at] == want[i]);
                CHECK(i == 0 || (out[at] > out[at - 1] && out[at] / tiles >= out[at - 1] / tiles));     // ascending, item-major
                ++at;
            }
            // valid frames of a prefix and of the slice behind it, counted frame by frame (every split of a short list, a few of a long one)
            long run = 0;
            const size_t nw = want.size(), step = nw <= 64 ? 1 : nw / 5;
            for (size_t i = 0; i <= nw; ++i) {
                if (i % step == 0 || i + 1 >= nw) {
                    CHECK(tile_frames(&g, g.T, BN, 0, (int)i) == (double)run);
                    CHECK(tile_frames(&g, g.T, BN, (int)i, (int)(nw - i)) == (double)(sum - run));
                }
                if (i == nw) break;
                const int b = want[i] / tiles, ft = want[i] % tiles;
                for (int t = ft * BN; t < (ft + 1) * BN; ++t) run += t < lens[b];
            }
            FullP fp = {};
            CHECK(fill_tiles(fp, &g, B, g.T, BN) == (long)want.size() && fp.tiles_per_b == tiles && fp.lens == g.lens &&
                  fp.cgmap == g.list[k] && fp.ncg == (int)want.size() && fp.inv_tiles_per_b == 1.0f / (float)tiles);
            BareP bp = {};
            CHECK(fill_tiles(bp, &g, B, g.T, BN) == (long)want.size() && bp.tiles_per_b == tiles && bp.cgmap == g.list[k]);
            TilesP tp = {};
            CHECK(fill_tiles(tp, &g, B, g.T, BN) == (long)want.size() && tp.tiles == tiles && tp.lens == g.lens);
            FullP dp = {};
            CHECK(fill_tiles(dp, nullptr, B, g.T, BN) == (long)B * tiles && dp.tiles_per_b == tiles && !dp.lens && !dp.cgmap && !dp.ncg);
        }
        CHECK(valid_frames(&g, B, g.T) == (double)sum && valid_frames(nullptr, B, g.T) == (double)B * g.T);
        if ((widths & (RAG_W16 | RAG_W32)) != (RAG_W16 | RAG_W32)) continue;
        // the 16-frame index of the first half of 32-frame tile n: the walk, and the same (item, frame) in both lists
        const int tpb16 = (g.T + 15) / 16, tpb32 = (g.T + 31) / 32;
        for (long n = 0; n <= g.count[1]; ++n) {
            const long m = rag_map16(&g, g.T, n);
            CHECK(m == map16_walk(lens, n));
            if (n == g.count[1]) { CHECK(m == g.count[0]); break; }
            const int e32 = g.list_host[1][n], e16 = g.list_host[0][m];
            CHECK(e16 / tpb16 == e32 / tpb32 && e16 % tpb16 == 2 * (e32 % tpb32));
        }
        for (long n = 0; n <= (long)B * tpb32; ++n) {       // dense: item b's tile j -> b * tpb16 + 2 j
            const long m = rag_map16(nullptr, g.T, n);
            CHECK(m == (n / tpb32) * tpb16 + 2 * (n % tpb32));
        }
    }
    CHECK(at == out.size());
}

int main() {
    const int Ts[] = {1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1000};
    const std::vector<long> one = {1}, voc = {1, 8, 64, 512};
    const unsigned den_w = RAG_W16 | RAG_W32 | RAG_W64, voc_w = RAG_W32 | RAG_W64 | RAG_W256;
    long batches = 0;
    auto run = [&](const std::vector<int>& lengths, int T) {
        for (unsigned w : {den_w, voc_w, den_w | voc_w})
            for (const std::vector<long>* m : {&one, &voc}) {
                check_batch(lengths, T, w, *m);
                ++batches;
            }
    };
    for (int T : Ts) {
        std::set<int> cs = {0, 1, T};       // the empty item, the one-frame item, the full one, and every boundary's neighbours
        for (int w : kRagWidths)
            for (int m = 1; m * w <= T + w; m = m == 1 ? 2 : m * 7)
                for (int d = -1; d <= 1; ++d)
                    if (m * w + d >= 0 && m * w + d <= T) cs.insert(m * w + d);
        const std::vector<int> cand(cs.begin(), cs.end());
        for (int v : cand) run({v}, T);                              // B = 1 (v = 0: all-empty)
        run(std::vector<int>(9, 0), T);                              // B = 9, all-empty
        for (size_t s = 0; s < cand.size(); ++s) {                   // B = 9: every window of the candidates ...
            std::vector<int> b9(9);
            for (int i = 0; i < 9; ++i) b9[i] = cand[(s + i) % cand.size()];
            run(b9, T);
            for (int z : {0, 4, 8}) {                                // ... with an empty item first, in the middle, last
                std::vector<int> e = b9;
                e[z] = 0;
                if (e[(z + 1) % 9] == 0) e[(z + 1) % 9] = 1;         // (beside a one-frame item)
                run(e, T);
            }
        }
    }
    printf("ragged_harness: %ld batches, %ld comparisons, all equal\n", batches, g_checks);
    return 0;
}
