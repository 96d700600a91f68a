// cop_fwd.hip — cop_fwd_mark / cop_fwd_write / cop_fwd_rw / cop_fwd_rw_status:
// the L3 forward step on forward lists and tx bursts (cop_fwd_check,
// cop_fwd_rewrite, include/cop_gpu.h "L3 forward"; host mirror: fwd.c).
//
// Both calls run on the chunk grid of cop_chunk.h.
//
// Check: cop_fwd_mark loads pieces 0..2 (bytes 0..47) of every entry's packet
// as the pipeline's loaders do, gathers results[i] (8 bytes) and the
// neighbour entry (one 16-byte load), and adds to the chunk's mark record its
// waves' TTL / NO_NEIGH counts and the 4-bit classes. cop_fwd_write, on the
// same grid, places the kept and the removed entries (a removed entry's place:
// the entries before it less the kept ones). Chunk 0 of a list writes status
// (and a dense list's counts); a segment's chunk writes its own count words.
// The classes are computed once, in the first kernel.
//
// Rewrite: cop_fwd_rw, one frame per lane. A chunk's first frame k0 is 256c
// or the sum of the earlier segments' counts (chunk_locate). A lane
// loads pieces 0 and 1 of its frame in the burst (piece 2 only to verify the
// checksum), classifies, and stores the two pieces of an OK frame: piece 0 is
// the entry's first three words and the frame's own fourth, piece 1 the
// frame's own with TTL and checksum replaced. Each chunk leaves its three
// counts in scratch; cop_fwd_rw_status, one workgroup per list, sums them in
// a fixed order into status.
//
// Only vector loads and stores, in plain C++.
//
// Bounds: the lists' are cop_chunk.h's; nh is compared with n_entries before
// the entry is loaded; W <= cap_frames, and a frame is touched only if its
// first 48 bytes lie, 16-byte aligned, inside cap_bytes (64-bit arithmetic);
// an IMIX packet of the check is read only if its clamped length is >= 34,
// which the caller backs with 48 readable bytes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cop_chunk.h"

namespace {

constexpr int BLOCK = CHUNK;
constexpr uint32_t SW = COPK_FWD_SCRATCH_WORDS;
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

enum : uint32_t { OK = 0, PASS = 1, SHORT = 2, BAD_HDR = 3, OPTIONS = 4, BAD_CSUM = 5, TTL = 6, NO_NEIGH = 7 };

__device__ __forceinline__ uint32_t fold16(uint32_t v)
{
    v = (v & 0xFFFFu) + (v >> 16);   // < 0x1FFFF for the sums here (at most 11 halves)
    v = (v & 0xFFFFu) + (v >> 16);
    return (v & 0xFFFFu) + (v >> 16);
}

__device__ __forceinline__ uint32_t halves(uint32_t w) { return (w & 0xFFFFu) + (w >> 16); }

// the class of a frame from its pieces as loaded (little-endian words); ent: the entry of an OK frame
__device__ __forceinline__ uint32_t class_of(const CopKFwdTab &t, const u32x4 &p0, const u32x4 &p1, uint32_t w8,
                                             const void *results, uint32_t i, u32x4 &ent)
{
    if ((p0.w & 0xFFFFu) != 0x0008u || ((p0.w >> 20) & 0xFu) != 4u) return PASS;
    const uint32_t ihl = (p0.w >> 16) & 0xFu;
    if (ihl < 5u) return BAD_HDR;
    if (ihl > 5u) return OPTIONS;
    if (t.verify) {
        // a one's complement sum does not depend on the byte order of its 16-bit words
        const uint32_t s = (p0.w >> 16) + halves(p1.x) + halves(p1.y) + halves(p1.z) + halves(p1.w) + (w8 & 0xFFFFu);
        if (fold16(s) != 0xFFFFu) return BAD_CSUM;
    }
    if (((p1.y >> 16) & 0xFFu) <= 1u) return TTL;
    uint32_t nh = t.miss_nh;
    if (results) {
        const u32x2 r = ((const u32x2 *)results)[i];
        if ((r.x >> 8) & COPK_FLAG_ROUTE_HIT) nh = r.y & 0xFFFFFFu;
    }
    if (nh >= t.n_entries) return NO_NEIGH;
    ent = *(const u32x4 *)(t.entries + 4 * (size_t)nh);
    return ((ent.w >> 16) & 1u) ? OK : NO_NEIGH;
}

__global__ __launch_bounds__(BLOCK) void cop_fwd_mark(const CopKFwd p)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const CopKFwdList &L = p.l[list_of(p, blockIdx.x)];
    const uint32_t c = blockIdx.x - L.h.chunk_begin;
    const uint32_t cnt = chunk_count(L.h, p.seg, c);
    uint32_t cls = 0xFu;   // no entry
    if ((uint32_t)tid < cnt) {
        const uint32_t i = chunk_entry(L.h, c, tid);
        bool is_short = false;
        const uint8_t *f;
        if (L.h.offsets) {
            is_short = min(max(L.lens[i], 1u), COPK_TX_MAX_FRAME) < 34u;
            f = L.h.pkts + (unsigned long long)L.h.offsets[i];
        } else {
            f = L.h.pkts + (unsigned long long)i * L.h.stride;
        }
        cls = SHORT;
        if (!is_short) {
            const u32x4 p0 = *(const u32x4 *)f, p1 = *(const u32x4 *)(f + 16), p2 = *(const u32x4 *)(f + 32);
            u32x4 ent;
            cls = class_of(p.tab, p0, p1, p2.x, L.results, i, ent);
        }
    }
    const unsigned long long ttl = __ballot(cls == TTL), nn = __ballot(cls == NO_NEIGH);
    // eight lanes' classes in one word
    uint32_t packed = cls << (4 * (lane & 7));
    packed |= __shfl_xor(packed, 1, 64);
    packed |= __shfl_xor(packed, 2, 64);
    packed |= __shfl_xor(packed, 4, 64);
    uint32_t *const sc = p.scratch + (size_t)(p.scratch_begin + blockIdx.x) * SW;
    if ((lane & 7) == 0) sc[24 + (tid >> 3)] = packed;
    if (lane == 0) {
        sc[16 + wave] = (uint32_t)__popcll(ttl);
        sc[20 + wave] = (uint32_t)__popcll(nn);
    }
    mark_put(sc, cls <= PASS, cnt);
}

__global__ __launch_bounds__(BLOCK) void cop_fwd_write(const CopKFwd p)
{
    __shared__ uint32_t red[4][4];
    const uint32_t tid = threadIdx.x;
    const CopKFwdList &L = p.l[list_of(p, blockIdx.x)];
    const uint32_t c = blockIdx.x - L.h.chunk_begin;
    const uint32_t *const sc0 = p.scratch + (size_t)(p.scratch_begin + L.h.chunk_begin) * SW;
    MarkAt m;
    uint32_t v[4] = {0u, 0u, 0u, 0u};   // {kept, entries, TTL, NO_NEIGH} of the chunks before this one; chunk 0: of every chunk
    if (!mark_get(sc0, SW, p.seg, c, (L.h.n + BLOCK - 1) / BLOCK, m, v, red, [](const uint32_t *x, uint32_t (&v)[4]) {
            const u32x4 t = *(const u32x4 *)(x + 16), nn = *(const u32x4 *)(x + 20);
            v[2] += t.x + t.y + t.z + t.w;
            v[3] += nn.x + nn.y + nn.z + nn.w;
        })) {
        if (p.seg && tid == 0) {
            L.out_count[c] = 0u;
            if (L.exc_count) L.exc_count[c] = 0u;
        }
        return;
    }
    if (c == 0 && tid == 0) {
        __builtin_nontemporal_store(u32x4{v[0], v[1] - v[0], v[2], v[3]}, (u32x4 *)L.status);
        if (!p.seg) {
            L.out_count[0] = v[0];
            if (L.exc_count) L.exc_count[0] = v[1] - v[0];
        }
    }
    if (p.seg && tid == 0) {
        L.out_count[c] = m.kept_here;
        if (L.exc_count) L.exc_count[c] = m.cnt - m.kept_here;
    }
    if (tid >= m.cnt) return;

    const uint32_t e = L.h.idx[(size_t)c * BLOCK + tid];
    if (m.keep) {
        L.out_idx[mark_base(p.seg, c, v[0]) + m.before] = e;
    } else if (L.exc_idx) {
        const uint32_t cls = (sc0[(size_t)c * SW + 24 + (tid >> 3)] >> (4 * (tid & 7))) & 0xFu;
        L.exc_idx[mark_base(p.seg, c, v[1] - v[0]) + (tid - m.before)] = min(e, L.h.n - 1u) | (cls << 28);
    }
}

__global__ __launch_bounds__(BLOCK) void cop_fwd_rw(const CopKFwd p)
{
    __shared__ uint32_t red[4][4];
    const int tid = threadIdx.x, lane = tid & 63;
    const CopKFwdList &L = p.l[list_of(p, blockIdx.x)];
    const uint32_t c = blockIdx.x - L.h.chunk_begin;
    const ChunkAt at = chunk_locate(L.h, p.seg, c, nullptr, red);
    const uint32_t cnt = at.cnt;
    const uint32_t W = min(min(L.tx_status[0], L.cap_frames), at.total);
    const uint32_t k = at.k0 + (uint32_t)tid;

    uint32_t cls = 0xFu;   // no frame
    if ((uint32_t)tid < cnt && k < W) {
        const uint32_t i = chunk_entry(L.h, c, tid);
        const unsigned long long fo = L.h.offsets ? (unsigned long long)L.off[k] : (unsigned long long)k * L.slot_bytes;
        bool is_short = (fo & 15ull) || fo + 48ull > (unsigned long long)L.cap_bytes;
        if (L.h.offsets && L.len[k] < 34u) is_short = true;
        cls = SHORT;
        u32x4 ent = {0u, 0u, 0u, 0u};
        if (!is_short) {
            uint8_t *const f = L.frames + fo;
            const u32x4 p0 = *(const u32x4 *)f, p1 = *(const u32x4 *)(f + 16);
            const uint32_t w8 = p.tab.verify ? *(const uint32_t *)(f + 32) : 0u;
            cls = class_of(p.tab, p0, p1, w8, L.results, i, ent);
            if (cls == OK) {
                // big-endian values of the words at bytes 22..23 and 24..25
                const uint32_t m = __builtin_bswap32(p1.y) & 0xFFFFu;
                const uint32_t hc = __builtin_bswap32(p1.z) >> 16;
                const uint32_t hc2 = ~fold16((~hc & 0xFFFFu) + (~m & 0xFFFFu) + (m - 0x0100u)) & 0xFFFFu;
                const uint32_t z = (p1.z & 0xFFFF0000u) | (hc2 >> 8) | ((hc2 & 0xFFu) << 8);
                *(u32x4 *)f = u32x4{ent.x, ent.y, ent.z, p0.w};
                *(u32x4 *)(f + 16) = u32x4{p1.x, p1.y - 0x00010000u, z, p1.w};
            }
        }
        if (L.port) L.port[k] = cls == OK ? (ent.w & 0xFFFFu) : 0xFFFFu;
    }
    const unsigned long long b_ok = __ballot(cls == OK), b_pass = __ballot(cls == PASS);
    const unsigned long long b_any = __ballot(cls != 0xFu);
    uint32_t v[4] = {0u, 0u, 0u, 0u};
    if (lane == 0) {
        v[0] = (uint32_t)__popcll(b_ok);
        v[1] = (uint32_t)__popcll(b_pass);
        v[2] = (uint32_t)__popcll(b_any) - v[0] - v[1];
    }
    block_sum(v, red);
    if (tid == 0)
        *(u32x4 *)(p.scratch + (size_t)(p.scratch_begin + blockIdx.x) * SW) = u32x4{v[0], v[1], v[2], 0u};
}

// one workgroup per list: its chunks' counts summed in a fixed order
__global__ __launch_bounds__(BLOCK) void cop_fwd_rw_status(const CopKFwd p)
{
    __shared__ uint32_t red[4][4];
    const int tid = threadIdx.x;
    const CopKFwdList &L = p.l[blockIdx.x];
    const uint32_t nchunk = (L.h.n + BLOCK - 1) / BLOCK;
    const uint32_t *const sc0 = p.scratch + (size_t)(p.scratch_begin + L.h.chunk_begin) * SW;
    uint32_t v[4] = {0u, 0u, 0u, 0u};
    for (uint32_t s = tid; s < nchunk; s += BLOCK) {
        const u32x4 x = *(const u32x4 *)(sc0 + (size_t)s * SW);
        v[0] += x.x;
        v[1] += x.y;
        v[2] += x.z;
    }
    block_sum(v, red);
    if (tid == 0) __builtin_nontemporal_store(u32x4{v[0], v[1], v[2], 0u}, (u32x4 *)L.status);
}

}  // namespace

extern "C" hipError_t copk_fwd_check_launch(const CopKFwd *pp, hipStream_t stream)
{
    const CopKFwd &p = *pp;
    if (!p.nl || !p.nchunks) return hipSuccess;
    if (p.nl > COPK_FWD_MAXL || !p.scratch || !p.tab.entries) return hipErrorInvalidValue;
    hipLaunchKernelGGL(cop_fwd_mark, dim3(p.nchunks), dim3(BLOCK), 0, stream, p);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    hipLaunchKernelGGL(cop_fwd_write, dim3(p.nchunks), dim3(BLOCK), 0, stream, p);
    return hipGetLastError();
}

extern "C" hipError_t copk_fwd_rewrite_launch(const CopKFwd *pp, hipStream_t stream)
{
    const CopKFwd &p = *pp;
    if (!p.nl || !p.nchunks) return hipSuccess;
    if (p.nl > COPK_FWD_MAXL || !p.scratch || !p.tab.entries) return hipErrorInvalidValue;
    hipLaunchKernelGGL(cop_fwd_rw, dim3(p.nchunks), dim3(BLOCK), 0, stream, p);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    hipLaunchKernelGGL(cop_fwd_rw_status, dim3(p.nl), dim3(BLOCK), 0, stream, p);
    return hipGetLastError();
}
