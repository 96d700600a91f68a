// cop_acl.hip — cop_acl_words / cop_acl_mark / cop_acl_write: the 5-tuple ACL
// over batches and forward lists (cop_acl_classify, cop_acl_filter,
// include/cop_gpu.h "ACL"; image and host mirror: acl.c).
//
// The word of a packet (acl_word, shared by both calls), 256 packets per
// workgroup, in three phases:
//   1. a packet per lane: the lane loads pieces 0..2 (bytes 0..47) of its
//      packet as the pipeline's loaders do and builds the key, while the
//      workgroup stages the four fields' interval starts in LDS (at most
//      4 x 2,049 words). Four binary searches there, at most 12 steps each,
//      give the interval ids; the word offsets of the packet's five rows go to
//      LDS.
//   2. eight lanes per packet, eight rounds of 32 packets: lane j loads 16
//      bytes of each of the five rows (a packet's row is one coalesced line of
//      up to 128 bytes, from L2), ANDs them and takes its own first set bit;
//      the minimum rank over the eight lanes by three __shfl_xor. Lanes at or
//      past row_words / 4 contribute nothing.
//   3. a packet per lane again: rank -> word from the rank table.
//
// Classify (cop_acl_words): the grid is sized from the batches' n, as the
// sketch update's. Filter: the chunk grid of cop_chunk.h and its mark record,
// as the police's two kernels; cop_acl_mark adds the waves' kept-as-miss and
// kept-as-skip counts to the record and counts the rules' hits: the chunk's
// hits per rule are summed in LDS (one word per rule; the lanes of a wave that
// hold its first hit's rule ride on that lane first), then every rule the
// chunk hit gets one u64 add in memory: exact, and a catch-all rule that every
// packet reaches costs a chunk one add (DESIGN.md 27.5 has the measurement).
// cop_acl_write places the kept entries. No other global atomics, and no
// workgroup waits for another.
//
// Only vector loads, stores and atomics, in plain C++ and __hip_atomic_*.
//
// Bounds: an interval id is below niv by the search, a protocol row below 256;
// a rank is read only below n_rules, a hit word written only for a rule index
// below n_rules; the lists' are cop_chunk.h's. All LDS of the kernels that
// call acl_word is dynamic, every part at a multiple of 16 bytes: the starts,
// the row offsets, the ranks and, in cop_acl_mark with counters, pad4(n_rules)
// hit words behind them.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cop_chunk.h"

namespace {

constexpr int BLOCK = CHUNK;
constexpr uint32_t SW = COPK_ACL_SCRATCH_WORDS;
constexpr uint32_t NONE = 0xFFFFFFFFu;
static_assert(COPK_ACL_CHUNK == CHUNK, "one chunk size");

__host__ __device__ inline uint32_t pad4(uint32_t w) { return (w + 3u) & ~3u; }

// dynamic LDS of a workgroup, in words: the four starts arrays, 5 x BLOCK row offsets, BLOCK ranks
__host__ __device__ inline uint32_t lds_words(const CopKAclTab &t)
{
    return pad4(t.niv[0]) + pad4(t.niv[1]) + pad4(t.niv[2]) + pad4(t.niv[3]) + 6u * BLOCK;
}

// the last j with s[j] <= k (s[0] == 0)
__device__ __forceinline__ uint32_t interval_of(const uint32_t *s, uint32_t niv, uint32_t k)
{
    uint32_t lo = 0, hi = niv;
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (s[mid] <= k) lo = mid;
        else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ uint32_t first_bit(const u32x4 &x, uint32_t j)
{
    if (x.x) return 128u * j + (uint32_t)__builtin_ctz(x.x);
    if (x.y) return 128u * j + 32u + (uint32_t)__builtin_ctz(x.y);
    if (x.z) return 128u * j + 64u + (uint32_t)__builtin_ctz(x.z);
    if (x.w) return 128u * j + 96u + (uint32_t)__builtin_ctz(x.w);
    return NONE;
}

// The word of this lane's packet i (has: the lane has one). Every thread of the workgroup calls it.
__device__ __forceinline__ uint32_t acl_word(const CopKAclTab &t, uint32_t *lds, const uint8_t *pkts,
                                             const uint32_t *offsets, uint32_t stride, bool has, uint32_t i)
{
    const uint32_t tid = threadIdx.x;
    u32x4 p0 = {}, p1 = {}, p2 = {};
    if (has) {
        const uint8_t *f = pkts + (offsets ? (unsigned long long)offsets[i] : (unsigned long long)i * stride);
        p0 = *(const u32x4 *)f, p1 = *(const u32x4 *)(f + 16), p2 = *(const u32x4 *)(f + 32);
    }
    // stage the starts: 16 bytes per lane, the arrays' pads included (the image holds them)
    uint32_t so[4], at = 0;
#pragma unroll
    for (int f = 0; f < 4; f++) {
        so[f] = at;
        const uint32_t quads = pad4(t.niv[f]) >> 2;
        const u32x4 *src = (const u32x4 *)(t.image + t.off_starts[f]);
        u32x4 *dst = (u32x4 *)(lds + at);
        for (uint32_t j = tid; j < quads; j += BLOCK) dst[j] = src[j];
        at += quads << 2;
    }
    uint32_t *const s_row = lds + at, *const s_rank = s_row + 5 * BLOCK;
    __syncthreads();

    // ---- 1: the key and its five rows ----
    const uint32_t ihl = (p0.w >> 16) & 0xFu;
    const bool skip = (p0.w & 0xFFFFu) != 0x0008u || ((p0.w >> 20) & 0xFu) != 4u || ihl < 5u;
    const bool live = has && !skip;
    if (live) {
        const uint32_t src = __builtin_bswap32((p1.z >> 16) | (p1.w << 16));
        const uint32_t dst = __builtin_bswap32((p1.w >> 16) | (p2.x << 16));
        const uint32_t proto = p1.y >> 24;
        const uint32_t frag = ((p1.y & 0x1Fu) << 8) | ((p1.y >> 8) & 0xFFu);
        uint32_t sport = 0, dport = 0;
        if (ihl == 5u && frag == 0u) {
            sport = ((p2.x >> 8) & 0xFF00u) | (p2.x >> 24);
            dport = ((p2.y << 8) & 0xFF00u) | ((p2.y >> 8) & 0xFFu);
        }
        const uint32_t key[4] = {src, dst, sport, dport};
#pragma unroll
        for (int f = 0; f < 4; f++)
            s_row[f * BLOCK + tid] = t.off_rows[f] + interval_of(lds + so[f], t.niv[f], key[f]) * t.row_words;
        s_row[4 * BLOCK + tid] = t.off_proto + proto * t.row_words;
    } else {
        s_row[tid] = NONE;
    }
    __syncthreads();

    // ---- 2: AND of the rows, first set bit ----
    const uint32_t j = tid & 7u, q = tid >> 3, quads = t.row_words >> 2;
#pragma unroll 4
    for (uint32_t r = 0; r < 8; r++) {
        const uint32_t pk = r * 32u + q;
        const uint32_t r0 = s_row[pk];
        uint32_t rank = NONE;
        if (r0 != NONE && j < quads) {
            u32x4 x = *(const u32x4 *)(t.image + r0 + 4u * j);
#pragma unroll
            for (int f = 1; f < 5; f++) x &= *(const u32x4 *)(t.image + s_row[f * BLOCK + pk] + 4u * j);
            rank = first_bit(x, j);
        }
        rank = min(rank, (uint32_t)__shfl_xor((int)rank, 1, 64));
        rank = min(rank, (uint32_t)__shfl_xor((int)rank, 2, 64));
        rank = min(rank, (uint32_t)__shfl_xor((int)rank, 4, 64));
        if (j == 0) s_rank[pk] = rank;
    }
    __syncthreads();

    // ---- 3: rank -> word ----
    if (!has) return 0u;
    if (skip) return COP_ACL_SKIP;
    const uint32_t rank = s_rank[tid];
    return rank < t.n_rules ? t.image[t.off_rank + rank] : 0u;
}

__global__ __launch_bounds__(BLOCK) void cop_acl_words(const CopKAclWords p)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const CopKAclBatch &B = p.b[item_of(p.nb, blockIdx.x, [&](uint32_t i) { return p.b[i].chunk_begin; })];
    const uint32_t i = (blockIdx.x - B.chunk_begin) * BLOCK + threadIdx.x;
    const bool has = i < B.n;
    const uint32_t w = acl_word(p.tab, lds, B.pkts, B.offsets, B.stride, has, i);
    if (has) B.words[i] = w;
}

__global__ __launch_bounds__(BLOCK) void cop_acl_mark(const CopKAcl p)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const CopKAclList &L = p.l[list_of(p, blockIdx.x)];
    const uint32_t c = blockIdx.x - L.h.chunk_begin;
    const uint32_t cnt = chunk_count(L.h, p.seg, c);
    uint32_t *const sc = p.scratch + (size_t)(p.scratch_begin + blockIdx.x) * SW;
    if (!cnt) {   // a chunk past its list's end, an empty segment: the same for every thread
        if (lane == 0) sc[16 + wave] = sc[20 + wave] = 0u;
        mark_put(sc, false, 0u);
        return;
    }
    const bool has = (uint32_t)tid < cnt;
    uint32_t *const s_hits = lds + lds_words(p.tab);   // one word per rule, with counters only
    if (p.tab.counters)
        for (uint32_t s = tid; s < p.tab.n_rules; s += BLOCK) s_hits[s] = 0u;   // acl_word's barriers order this
    const uint32_t w = acl_word(p.tab, lds, L.h.pkts, L.h.offsets, L.h.stride, has, has ? chunk_entry(L.h, c, tid) : 0u);
    const bool keep = has && !(w & COP_ACL_DROP);

    if (p.tab.counters) {
        // the chunk's hits per rule in LDS, then one global add per rule the chunk hit: exact, every hit
        // adds 1 to one LDS word and every non-zero word reaches memory once
        const bool hit = has && (w & COP_ACL_HIT) && (w & 0x00FFFFFFu) < p.tab.n_rules;
        const uint32_t rule = w & 0x00FFFFFFu;
        uint32_t mine = hit ? 1u : 0u;
        const unsigned long long m = __ballot(hit);
        if (m) {   // the lanes that hold the wave's first hit's rule ride on that lane
            const int leader = __ffsll((long long)m) - 1;
            const bool eq = hit && rule == (uint32_t)__shfl((int)rule, leader, 64);
            const unsigned long long same = __ballot(eq);
            if (eq) mine = lane == leader ? (uint32_t)__popcll(same) : 0u;
        }
        if (mine) atomicAdd(&s_hits[rule], mine);
        __syncthreads();
        for (uint32_t s = tid; s < p.tab.n_rules; s += BLOCK) {
            const uint32_t h = s_hits[s];
            if (h)
                (void)__hip_atomic_fetch_add(&p.tab.counters[s], (unsigned long long)h, __ATOMIC_RELAXED,
                                             __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    const unsigned long long miss = __ballot(keep && w == 0u), skipped = __ballot(keep && w == COP_ACL_SKIP);
    if (lane == 0) {
        sc[16 + wave] = (uint32_t)__popcll(miss);
        sc[20 + wave] = (uint32_t)__popcll(skipped);
    }
    mark_put(sc, keep, cnt);
}

__global__ __launch_bounds__(BLOCK) void cop_acl_write(const CopKAcl p)
{
    __shared__ uint32_t red[4][4];
    const uint32_t tid = threadIdx.x;
    const CopKAclList &L = p.l[list_of(p, blockIdx.x)];
    const uint32_t c = blockIdx.x - L.h.chunk_begin;
    MarkAt m;
    uint32_t v[4] = {0u, 0u, 0u, 0u};   // {kept, entries, miss, skip} of the chunks before this one; chunk 0: of every chunk
    if (!mark_get(p.scratch + (size_t)(p.scratch_begin + L.h.chunk_begin) * SW, SW, p.seg, c, (L.h.n + BLOCK - 1) / BLOCK,
                  m, v, red, [](const uint32_t *x, uint32_t (&v)[4]) {
                      const u32x4 a = *(const u32x4 *)(x + 16), b = *(const u32x4 *)(x + 20);
                      v[2] += a.x + a.y + a.z + a.w;
                      v[3] += b.x + b.y + b.z + b.w;
                  })) {
        if (p.seg && tid == 0) L.out_count[c] = 0u;
        return;
    }
    if (c == 0 && tid == 0) {
        __builtin_nontemporal_store(u32x4{v[0], v[1] - v[0], v[2], v[3]}, (u32x4 *)L.status);
        if (!p.seg) L.out_count[0] = v[0];
    }
    if (p.seg && tid == 0) L.out_count[c] = m.kept_here;
    if (tid < m.cnt && m.keep) L.out_idx[mark_base(p.seg, c, v[0]) + m.before] = L.h.idx[(size_t)c * BLOCK + tid];
}

}  // namespace

extern "C" hipError_t copk_acl_words_launch(const CopKAclWords *pp, hipStream_t stream)
{
    const CopKAclWords &p = *pp;
    if (!p.nb || !p.nchunks) return hipSuccess;
    if (p.nb > COPK_ACL_MAXB || !p.tab.image || (p.tab.row_words & 3u) || p.tab.row_words > 32u)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(cop_acl_words, dim3(p.nchunks), dim3(BLOCK), lds_words(p.tab) * 4u, stream, p);
    return hipGetLastError();
}

extern "C" hipError_t copk_acl_filter_launch(const CopKAcl *pp, hipStream_t stream)
{
    const CopKAcl &p = *pp;
    if (!p.nl || !p.nchunks) return hipSuccess;
    if (p.nl > COPK_ACL_MAXL || !p.scratch || !p.tab.image || (p.tab.row_words & 3u) || p.tab.row_words > 32u)
        return hipErrorInvalidValue;
    const uint32_t words = lds_words(p.tab) + (p.tab.counters ? pad4(p.tab.n_rules) : 0u);   // + the chunk's hits per rule
    hipLaunchKernelGGL(cop_acl_mark, dim3(p.nchunks), dim3(BLOCK), words * 4u, stream, p);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    hipLaunchKernelGGL(cop_acl_write, dim3(p.nchunks), dim3(BLOCK), 0, stream, p);
    return hipGetLastError();
}
