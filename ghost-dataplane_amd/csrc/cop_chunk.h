// cop_chunk.h — the chunk grid the side calls' kernels run on (cop_tx.hip,
// cop_sketch.hip, cop_fwd.hip; cop_aead.hip takes the reduction and the walk).
// Device code only.
//
// The host does not know the list lengths, so a grid is sized from n: one
// workgroup of CHUNK threads per chunk of CHUNK consecutive positions of one
// forward list (a segment of a segmented list; positions 256c .. of a dense or
// per-vport list), workgroup chunk_begin + c serving its list's chunk c. A
// chunk past its list's end leaves after reading the count. No atomics, and no
// workgroup waits for another:
//   - a chunk's first list position is 256c (dense, per vport) or the sum of
//     the earlier segments' counts, read and reduced inside the workgroup (at
//     most 1,024 words for a 262,144-packet batch, from L2): chunk_locate;
//   - a call that removes entries runs two kernels on the same grid. The first
//     leaves every chunk's mark record in context-owned scratch (mark_put): the
//     waves' keep ballots, their kept counts and the chunk's length. The second
//     (mark_get) places the entries: a chunk's output base is the sum of the
//     earlier chunks' kept counts (dense, per vport) or the segment's own
//     start, a lane's place the kept bits below it. Chunk 0 of a list, which
//     exists for every list, sums all chunks, for the list's status.
//
// Bounds: an index >= n is read as n - 1; a count is clamped to what the
// layout holds, so a kept entry's place is below the list's (segment's)
// capacity.
#ifndef COP_CHUNK_H
#define COP_CHUNK_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cop_gpu.h"
#include "cop_kernels.h"

namespace {

constexpr int CHUNK = COPK_CHUNK;
static_assert(COPK_TX_CHUNK == CHUNK && COPK_SK_CHUNK == CHUNK && COPK_FWD_CHUNK == CHUNK && COP_SEG_PKTS == CHUNK,
              "one chunk size for every side call and the segments");
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ uint32_t wave_sum(uint32_t v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// sums of N values over the workgroup's four waves (every thread gets them)
template <int N>
__device__ __forceinline__ void block_sum(uint32_t (&v)[N], uint32_t (*red)[N])
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int j = 0; j < N; j++) v[j] = wave_sum(v[j]);
    __syncthreads();   // red may still be read from an earlier use
    if (lane == 0)
#pragma unroll
        for (int j = 0; j < N; j++) red[wave][j] = v[j];
    __syncthreads();
#pragma unroll
    for (int j = 0; j < N; j++) v[j] = red[0][j] + red[1][j] + red[2][j] + red[3][j];
}

// the item (list, batch, burst) of workgroup wg: the last of n_items whose first workgroup, begin_of(i), is <= wg
template <typename F>
__device__ __forceinline__ uint32_t item_of(uint32_t n_items, uint32_t wg, F begin_of)
{
    uint32_t i = 0;
    while (i + 1 < n_items && wg >= begin_of(i + 1)) i++;
    return i;
}

// the list of this workgroup, of a launch's p.nl lists p.l[]
template <typename P>
__device__ __forceinline__ uint32_t list_of(const P &p, uint32_t wg)
{
    return item_of(p.nl, wg, [&](uint32_t i) { return p.l[i].h.chunk_begin; });
}

// positions chunk c has in the layout of a batch of n packets
__device__ __forceinline__ uint32_t chunk_cap(uint32_t n, uint32_t c)
{
    const uint32_t first = c * CHUNK;
    return n > first ? min(n - first, (uint32_t)CHUNK) : 0u;
}

// entries of chunk c of a list
__device__ __forceinline__ uint32_t chunk_count(const CopKListHead &h, uint32_t seg, uint32_t c)
{
    if (seg) return min(h.count[c], chunk_cap(h.n, c));
    return chunk_cap(min(h.count[0], h.n), c);
}

// the packet of the chunk's entry t (below its count)
__device__ __forceinline__ uint32_t chunk_entry(const CopKListHead &h, uint32_t c, uint32_t t)
{
    return min(h.idx[(size_t)c * CHUNK + t], h.n - 1u);
}

// Where chunk c lies in its list: its entries cnt, its first list position k0 and the list's length
// total. A segmented list's k0 is a reduction over the segments' counts; `extra` (or null) is one
// word per chunk that the same reduction sums over the chunks before c, into extra_before.
struct ChunkAt {
    uint32_t cnt, k0, total, extra_before;
};
template <int N>
__device__ __forceinline__ ChunkAt chunk_locate(const CopKListHead &h, uint32_t seg, uint32_t c, const uint32_t *extra,
                                                uint32_t (*red)[N])
{
    static_assert(N >= 3, "three sums");
    ChunkAt at;
    if (seg) {
        const uint32_t nchunk = (h.n + CHUNK - 1) / CHUNK;
        uint32_t v[N] = {};
        for (uint32_t s = threadIdx.x; s < nchunk; s += CHUNK) {
            const uint32_t x = min(h.count[s], chunk_cap(h.n, s));
            v[0] += x;
            if (s < c) {
                v[1] += x;
                if (extra) v[2] += extra[s];
            }
        }
        block_sum(v, red);
        at.cnt = min(h.count[c], chunk_cap(h.n, c));
        at.total = v[0];
        at.k0 = v[1];
        at.extra_before = v[2];
    } else {
        at.total = min(h.count[0], h.n);
        at.k0 = c * CHUNK;
        at.cnt = chunk_cap(at.total, c);
        at.extra_before = 0;
    }
    return at;
}

// ---- the mark record of a chunk: words 0..7 the four waves' keep ballots, 8..11 their kept counts,
// 12 the chunk's entries (a kernel's further words from 16 on) ----------------------------------------
__device__ __forceinline__ void mark_put(uint32_t *sc, bool keep, uint32_t cnt)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long bits = __ballot(keep);
    if (lane == 0) {
        sc[2 * wave] = (uint32_t)bits;
        sc[2 * wave + 1] = (uint32_t)(bits >> 32);
        sc[8 + wave] = (uint32_t)__popcll(bits);
    }
    if (threadIdx.x == 0) sc[12] = cnt;
}

// What the placing kernel reads of the records (sw words each) of a list, sc0 its chunk 0's:
// false for a chunk past the list's end or an empty segment (cnt == 0, c != 0), which has nothing to
// place. Else the lane's keep bit and the kept entries before it in the chunk, the chunk's kept
// entries, and in v the sums over the chunks before c (chunk 0: over every chunk; a segmented list's
// other chunks need none): v[0] kept, v[1] entries, and what more(record, v) adds to the rest.
struct MarkAt {
    uint32_t cnt, before, kept_here;
    bool keep;
};
template <int N, typename F>
__device__ __forceinline__ bool mark_get(const uint32_t *sc0, uint32_t sw, uint32_t seg, uint32_t c, uint32_t nchunk,
                                         MarkAt &m, uint32_t (&v)[N], uint32_t (*red)[N], F more)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t *const sc = sc0 + (size_t)c * sw;
    m.cnt = sc[12];
    if (!m.cnt && c != 0) return false;
    if (c == 0 || !seg) {
        const uint32_t upto = c ? c : nchunk;
        for (uint32_t s = threadIdx.x; s < upto; s += CHUNK) {
            const uint32_t *const x = sc0 + (size_t)s * sw;
            const u32x4 k = *(const u32x4 *)(x + 8);
            v[0] += k.x + k.y + k.z + k.w;
            v[1] += x[12];
            more(x, v);
        }
        block_sum(v, red);
    }
    const u32x4 wk = *(const u32x4 *)(sc + 8);
    const unsigned long long bits = ((unsigned long long)sc[2 * wave + 1] << 32) | sc[2 * wave];
    m.kept_here = wk.x + wk.y + wk.z + wk.w;
    m.keep = (bits >> lane) & 1ull;
    m.before = (wave > 0 ? wk.x : 0u) + (wave > 1 ? wk.y : 0u) + (wave > 2 ? wk.z : 0u) +
               (uint32_t)__popcll(bits & ((1ull << lane) - 1ull));
    return true;
}

// first output position of chunk c: the segment's own start, or the entries placed by the chunks before it
__device__ __forceinline__ size_t mark_base(uint32_t seg, uint32_t c, uint32_t placed_before)
{
    return seg ? (size_t)c * CHUNK : (size_t)(c ? placed_before : 0u);
}

}  // namespace

#endif
