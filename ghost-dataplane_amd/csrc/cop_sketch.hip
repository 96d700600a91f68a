// cop_sketch.hip — cop_sketch_add / cop_sketch_est / cop_sketch_pol_mark /
// cop_sketch_pol_write / cop_sketch_decay: a count-min sketch of the traffic in
// device memory (cop_sketch_*, include/cop_gpu.h; host mirror: sketch.c).
//
// Update (cop_sketch_add): one packet per lane, 256 per workgroup, the grid
// sized from the batches' n. A lane loads the 16-byte pieces that hold
// EtherType / version / src / dst (bytes 0..47 of a frame, the one piece of a
// 16-byte record), as the pipeline's loaders do, and derives its key. The
// counters are then bumped with non-returning 64-bit adds at agent scope, up
// to `rows` per packet on scattered words. A heavy hitter would put every lane
// of a workgroup on the same `rows` words, so equal keys are combined first,
// exactly: (1) a wave whose counting lanes mostly hold the first such lane's
// key lets that lane carry their number (one ballot, no memory); (2) what is
// left goes into a 512-slot LDS table of the workgroup (open addressing, a
// 64-bit compare-and-swap on {1, key} claims a slot, an LDS add counts; 256
// lanes can never fill 512 slots); (3) every occupied slot issues `rows`
// global adds of its summed count. The count is exact: every counting lane
// adds 1 to exactly one slot, and every slot's sum reaches memory once.
//
// Query (cop_sketch_est): one address per lane, a gather of `rows` words.
//
// Police: the chunk grid of cop_chunk.h and its mark record.
// cop_sketch_pol_mark looks every entry's packet up and marks the entries to
// keep; cop_sketch_pol_write, on the same grid, places them. Chunk 0 of a list
// writes status (and a dense list's out_count); a segment's chunk writes its
// out_count word. The estimates are computed once, in the first kernel.
//
// Decay (cop_sketch_decay): a 16-byte-per-lane sweep.
//
// Only vector loads, stores and atomics, in plain C++ and __hip_atomic_*.
//
// Bounds: a column is below cols by its shift, a row below rows <= 4; the
// lists' are cop_chunk.h's.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cop_chunk.h"

namespace {

constexpr int BLOCK = CHUNK;
constexpr uint32_t SLOTS = 512;
typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ uint32_t col_of(const CopKSketch &s, uint32_t r, uint32_t k)
{
    return (uint32_t)(k * s.a[r] + s.b[r]) >> s.col_shift;
}

__device__ __forceinline__ unsigned long long est_of(const CopKSketch &s, uint32_t k)
{
    unsigned long long e = ~0ull;
    for (uint32_t r = 0; r < s.rows; r++) {
        const unsigned long long v = s.ctr[((size_t)r << s.log2_cols) + col_of(s, r, k)];
        e = v < e ? v : e;
    }
    return e;
}

// packet i: true and the key if it counts as IPv4 (the pipeline's two checks on the same bytes)
__device__ __forceinline__ bool packet_key(const CopKSketch &s, const uint8_t *pkts, const uint32_t *offsets,
                                           uint32_t stride, uint32_t i, uint32_t &key)
{
    const uint8_t *p = pkts + (offsets ? (unsigned long long)offsets[i] : (unsigned long long)i * stride);
    uint32_t w3, w6, w7, w8;   // frame bytes 12..15 and 24..35 as loaded (LE)
    if (!offsets && stride == 16u) {
        const u32x4 r = *(const u32x4 *)p;
        w3 = r.x, w6 = r.y, w7 = r.z, w8 = r.w;
    } else {
        const u32x4 p0 = *(const u32x4 *)p, p1 = *(const u32x4 *)(p + 16), p2 = *(const u32x4 *)(p + 32);
        w3 = p0.w, w6 = p1.z, w7 = p1.w, w8 = p2.x;
    }
    const uint32_t et = ((w3 & 0xFFu) << 8) | ((w3 >> 8) & 0xFFu);
    const uint32_t addr = s.dst ? __builtin_bswap32((w7 >> 16) | (w8 << 16)) : __builtin_bswap32((w6 >> 16) | (w7 << 16));
    key = addr >> s.key_shift;
    return et == 0x0800u && ((w3 >> 20) & 0xFu) == 4u;
}

__device__ __forceinline__ void add_rows(const CopKSketch &s, uint32_t k, unsigned long long v)
{
    for (uint32_t r = 0; r < s.rows; r++)
        (void)__hip_atomic_fetch_add(&s.ctr[((size_t)r << s.log2_cols) + col_of(s, r, k)], v, __ATOMIC_RELAXED,
                                     __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(BLOCK) void cop_sketch_add(const CopKSkUpdate p)
{
    __shared__ unsigned long long s_key[SLOTS];   // 0: free; else 1 << 32 | key
    __shared__ uint32_t s_cnt[SLOTS];
    const int tid = threadIdx.x, lane = tid & 63;
    const CopKSkBatch &B = p.b[item_of(p.nb, blockIdx.x, [&](uint32_t i) { return p.b[i].chunk_begin; })];
    const uint32_t i = (blockIdx.x - B.chunk_begin) * BLOCK + (uint32_t)tid;

    bool counts = false;
    uint32_t key = 0;
    if (i < B.n) {
        bool ok = true;
        if (p.verdict_mask) {
            const uint32_t v = ((const uint32_t *)B.results)[2 * (size_t)i] & 0xFFu;
            ok = v < 32u && ((p.verdict_mask >> v) & 1u);
        }
        if (ok) counts = packet_key(p.sk, B.pkts, B.offsets, B.stride, i, key);
    }
    if (!p.combine) {
        if (counts) add_rows(p.sk, key, 1ull);
        return;
    }

    for (uint32_t s = tid; s < SLOTS; s += BLOCK) {
        s_key[s] = 0ull;
        s_cnt[s] = 0u;
    }
    __syncthreads();
    // (1) the wave's lanes that hold its first counting lane's key ride on that lane
    uint32_t mine = counts ? 1u : 0u;
    const unsigned long long m = __ballot(counts);
    if (m) {
        const int leader = __ffsll((long long)m) - 1;
        const uint32_t k0 = (uint32_t)__shfl((int)key, leader, 64);
        const bool eq = counts && key == k0;
        const unsigned long long same = __ballot(eq);
        if (eq) mine = lane == leader ? (uint32_t)__popcll(same) : 0u;
    }
    // (2) the workgroup's table
    if (mine) {
        const unsigned long long tag = (1ull << 32) | key;
        uint32_t s = (key * 0x9E3779B1u) >> 23;
        for (;;) {
            const unsigned long long prev = atomicCAS(&s_key[s], 0ull, tag);
            if (prev == 0ull || prev == tag) break;
            s = (s + 1u) & (SLOTS - 1u);
        }
        atomicAdd(&s_cnt[s], mine);
    }
    __syncthreads();
    // (3) one global add per distinct key and row
    for (uint32_t s = tid; s < SLOTS; s += BLOCK) {
        const uint32_t c = s_cnt[s];
        if (c) add_rows(p.sk, (uint32_t)s_key[s], (unsigned long long)c);
    }
}

__global__ __launch_bounds__(BLOCK) void cop_sketch_est(const CopKSketch s, const uint32_t *__restrict__ ips, uint32_t n,
                                                        unsigned long long *__restrict__ out)
{
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i < n) out[i] = est_of(s, ips[i] >> s.key_shift);
}

__global__ __launch_bounds__(BLOCK) void cop_sketch_decay(const CopKSketch s, uint32_t shift)
{
    const size_t pairs = ((size_t)s.rows << s.log2_cols) >> 1;   // cols >= 16: the words are even in number
    u64x2 *const w = (u64x2 *)s.ctr;
    for (size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x; i < pairs; i += (size_t)gridDim.x * BLOCK) {
        u64x2 v = w[i];
        if (shift >= 64u) v = u64x2{0ull, 0ull};
        else v = u64x2{v.x >> shift, v.y >> shift};
        w[i] = v;
    }
}

// ---- police -------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void cop_sketch_pol_mark(const CopKSkPolice p)
{
    const CopKSkList &L = p.l[list_of(p, blockIdx.x)];
    const uint32_t c = blockIdx.x - L.h.chunk_begin;
    const uint32_t cnt = chunk_count(L.h, p.seg, c);
    bool keep = false;
    if (threadIdx.x < cnt) {
        uint32_t key;
        keep = !packet_key(p.sk, L.h.pkts, L.h.offsets, L.h.stride, chunk_entry(L.h, c, threadIdx.x), key) ||
               est_of(p.sk, key) < L.threshold;
    }
    mark_put(p.scratch + (size_t)(p.scratch_begin + blockIdx.x) * COPK_SK_SCRATCH_WORDS, keep, cnt);
}

__global__ __launch_bounds__(BLOCK) void cop_sketch_pol_write(const CopKSkPolice p)
{
    __shared__ uint32_t red[4][2];
    const uint32_t tid = threadIdx.x;
    const CopKSkList &L = p.l[list_of(p, blockIdx.x)];
    const uint32_t c = blockIdx.x - L.h.chunk_begin;
    MarkAt m;
    uint32_t v[2] = {0u, 0u};   // kept and entries of the chunks before this one; chunk 0: of every chunk
    if (!mark_get(p.scratch + (size_t)(p.scratch_begin + L.h.chunk_begin) * COPK_SK_SCRATCH_WORDS, COPK_SK_SCRATCH_WORDS,
                  p.seg, c, (L.h.n + BLOCK - 1) / BLOCK, m, v, red, [](const uint32_t *, uint32_t (&)[2]) {})) {
        if (p.seg && tid == 0) L.out_count[c] = 0u;
        return;
    }
    if (c == 0 && tid == 0) {
        __builtin_nontemporal_store(u32x4{v[0], v[1] - v[0], 0u, 0u}, (u32x4 *)L.status);
        if (!p.seg) L.out_count[0] = v[0];
    }
    if (p.seg && tid == 0) L.out_count[c] = m.kept_here;
    if (tid < m.cnt && m.keep) L.out_idx[mark_base(p.seg, c, v[0]) + m.before] = L.h.idx[(size_t)c * BLOCK + tid];
}

}  // namespace

extern "C" hipError_t copk_sketch_update_launch(const CopKSkUpdate *pp, hipStream_t stream)
{
    const CopKSkUpdate &p = *pp;
    if (!p.nb || !p.nchunks) return hipSuccess;
    if (p.nb > COPK_SK_MAXB || !p.sk.ctr) return hipErrorInvalidValue;
    hipLaunchKernelGGL(cop_sketch_add, dim3(p.nchunks), dim3(BLOCK), 0, stream, p);
    return hipGetLastError();
}

extern "C" hipError_t copk_sketch_police_launch(const CopKSkPolice *pp, hipStream_t stream)
{
    const CopKSkPolice &p = *pp;
    if (!p.nl || !p.nchunks) return hipSuccess;
    if (p.nl > COPK_SK_MAXL || !p.scratch || !p.sk.ctr) return hipErrorInvalidValue;
    hipLaunchKernelGGL(cop_sketch_pol_mark, dim3(p.nchunks), dim3(BLOCK), 0, stream, p);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    hipLaunchKernelGGL(cop_sketch_pol_write, dim3(p.nchunks), dim3(BLOCK), 0, stream, p);
    return hipGetLastError();
}

extern "C" hipError_t copk_sketch_query_launch(const CopKSketch *sk, const uint32_t *ips, uint32_t n,
                                               unsigned long long *out, hipStream_t stream)
{
    if (!n) return hipSuccess;
    if (!sk->ctr) return hipErrorInvalidValue;
    hipLaunchKernelGGL(cop_sketch_est, dim3((n + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, stream, *sk, ips, n, out);
    return hipGetLastError();
}

extern "C" hipError_t copk_sketch_decay_launch(const CopKSketch *sk, uint32_t shift, hipStream_t stream)
{
    if (!sk->ctr) return hipErrorInvalidValue;
    const size_t pairs = ((size_t)sk->rows << sk->log2_cols) >> 1;
    const uint32_t grid = (uint32_t)((pairs + BLOCK - 1) / BLOCK < 4096 ? (pairs + BLOCK - 1) / BLOCK : 4096);
    hipLaunchKernelGGL(cop_sketch_decay, dim3(grid), dim3(BLOCK), 0, stream, *sk, shift);
    return hipGetLastError();
}
