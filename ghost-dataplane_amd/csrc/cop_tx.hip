// cop_tx.hip — cop_tx_sums / cop_tx_copy: forwarded frames packed into tx
// bursts (cop_tx_gather, include/cop_gpu.h; host mirror: tx_gather.c).
//
// The kernels run on the chunk grid of cop_chunk.h: one workgroup per 256
// consecutive positions of one list, no atomics, no workgroup waiting for
// another. Where a chunk's frames go:
//   - a slot batch's byte offsets are arithmetic (k * slot_bytes);
//   - an IMIX batch's chunk starts at the sum of the earlier chunks' extents:
//     cop_tx_sums, a pre-pass on the same grid, writes each chunk's byte sum to
//     context-owned scratch, cop_tx_copy sums the entries before its own (in
//     the reduction that finds a segmented chunk's place) and scans inside the
//     chunk.
//
// status is written by exactly one chunk of every list, which finds out by
// itself that it is the one: the chunk holding the first frame that does not
// fit (every earlier frame fits iff the frame before the chunk does, which
// the chunk's own base position and byte base tell), or else the chunk
// holding the list's last position (an empty list's chunk 0).
//
// Copies: every lane moves 16 bytes, four pieces in flight per lane. Piece q
// of a chunk is piece q % P of frame q / P for a slot batch (P = copy_bytes /
// 16: a 64-byte frame takes 4 lanes, so a wave instruction reads 16 whole
// frames and writes 1 KiB contiguous when slot_bytes == copy_bytes; a
// 1,024-byte frame is one wave instruction). An IMIX chunk's output is
// contiguous by construction (extents are multiples of 16), so piece q goes to
// chunk base + 16 q and its frame is found by a binary search over the chunk's
// 256 offsets in LDS (8 steps): a wave instruction always writes 1 KiB
// contiguous, whatever the frame lengths. Loads and stores are non-temporal:
// no byte is touched twice. Only vector stores.
//
// Bounds: an index >= n is read as n - 1; a count is clamped to what the
// layout holds; a frame is stored only if it ends inside cap_bytes and its
// position is below cap_frames, in 64-bit arithmetic.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cop_chunk.h"

namespace {

constexpr int BLOCK = CHUNK;

__device__ __forceinline__ uint32_t frame_ext(uint32_t len, uint32_t &l)
{
    l = min(max(len, 1u), COPK_TX_MAX_FRAME);
    return (l + 15u) & ~15u;
}

// IMIX pre-pass: sums[sums_begin + c] = the bytes chunk c's frames take
__global__ __launch_bounds__(BLOCK) void cop_tx_sums(const CopKTx p)
{
    __shared__ uint32_t red[4][3];
    const int tid = threadIdx.x;
    const CopKTxList &L = p.l[list_of(p, blockIdx.x)];
    const uint32_t c = blockIdx.x - L.h.chunk_begin;
    if (!L.h.n) return;
    const uint32_t cnt = chunk_count(L.h, p.seg, c);
    if (!cnt && !p.seg) return;
    uint32_t v[3] = {0u, 0u, 0u};
    if ((uint32_t)tid < cnt) {
        uint32_t l;
        v[0] = frame_ext(L.lens[chunk_entry(L.h, c, tid)], l);
    }
    block_sum(v, red);
    if (tid == 0) p.sums[L.sums_begin + c] = v[0];
}

template <bool IMIX>
__global__ __launch_bounds__(BLOCK) void cop_tx_copy(const CopKTx p)
{
    __shared__ uint32_t red[4][3];
    __shared__ uint32_t s_src[BLOCK];       // slot: packet index; IMIX: offsets[i]
    __shared__ uint32_t s_off[BLOCK + 1];   // IMIX: byte offset inside the chunk; [cnt] = the chunk's bytes
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const CopKTxList &L = p.l[list_of(p, blockIdx.x)];
    const uint32_t c = blockIdx.x - L.h.chunk_begin;
    if (!L.h.n) {   // an empty batch: one chunk, a zero status
        if (tid == 0) __builtin_nontemporal_store(u32x4{0u, 0u, 0u, 0u}, (u32x4 *)L.status);
        return;
    }

    // the chunk's frames, its first list position k0, the list's length, the chunk's byte base (IMIX)
    const uint32_t *const sums = IMIX ? p.sums + L.sums_begin : nullptr;
    const ChunkAt at = chunk_locate(L.h, p.seg, c, sums, red);
    const uint32_t cnt = at.cnt, k0 = at.k0, total = at.total;
    uint32_t bytes0 = at.extra_before;
    if (!p.seg) {
        if (!cnt && c != 0) return;   // past the list's end
        if (IMIX) {
            uint32_t v[3] = {0u, 0u, 0u};
            for (uint32_t s = tid; s < c; s += BLOCK) v[0] += sums[s];
            block_sum(v, red);
            bytes0 = v[0];
        }
    }

    // one frame per thread: source, extent, offset, whether it fits
    const uint32_t k = k0 + (uint32_t)tid;
    uint32_t ext = 0, len = 0, off = 0, src = 0;
    if ((uint32_t)tid < cnt) {
        const uint32_t i = chunk_entry(L.h, c, tid);
        if (IMIX) {
            ext = frame_ext(L.lens[i], len);
            src = L.h.offsets[i];
        } else {
            ext = len = L.copy_bytes;
            src = i;
        }
    }
    unsigned long long off64;
    if (IMIX) {
        // exclusive scan of ext over the workgroup
        uint32_t inc = ext;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t t = __shfl_up(inc, d, 64);
            if (lane >= d) inc += t;
        }
        __syncthreads();
        if (lane == 63) red[wave][0] = inc;
        __syncthreads();
        uint32_t wpre = 0;
        for (int w = 0; w < wave; w++) wpre += red[w][0];
        const uint32_t excl = wpre + inc - ext;
        s_off[tid] = excl;
        if ((uint32_t)tid + 1u == cnt) s_off[cnt] = excl + ext;
        off = bytes0 + excl;
        off64 = off;
    } else {
        off64 = (unsigned long long)k * L.slot_bytes;
        off = (uint32_t)off64;
    }
    s_src[tid] = src;
    const bool fits = (uint32_t)tid < cnt && k < L.cap_frames && off64 + ext <= (unsigned long long)L.cap_bytes;
    // fits is monotone in the position: w = the frames of this chunk that are written
    uint32_t fit[3] = {fits ? 1u : 0u, 0u, 0u};
    block_sum(fit, red);   // (its barriers also publish s_src / s_off)
    const uint32_t w = fit[0];
    if (fits) {
        if (L.off) L.off[k] = off;
        if (L.len) L.len[k] = len;
    }

    // status: the chunk with the first frame that does not fit, else the one with the last position
    {
        const unsigned long long base64 =
            IMIX ? (unsigned long long)bytes0
                 : (k0 ? (unsigned long long)(k0 - 1u) * L.slot_bytes + L.copy_bytes : 0ull);
        const bool reached = k0 == 0 || (k0 <= L.cap_frames && base64 <= (unsigned long long)L.cap_bytes);
        const bool last = p.seg ? ((cnt > 0 && k0 + cnt == total) || (total == 0 && c == 0)) : (k0 + cnt == total);
        if (reached && (w < cnt || last) && (uint32_t)tid == (w ? w - 1u : 0u)) {
            const uint32_t used = w ? off + ext : (uint32_t)base64;   // thread w - 1 holds the last written frame
            __builtin_nontemporal_store(u32x4{k0 + w, used, total - (k0 + w), 0u}, (u32x4 *)L.status);
        }
    }
    if (!w) return;

    // the copy: 16 bytes per lane, four pieces in flight
    const uint8_t *const pk = L.h.pkts;
    uint8_t *const out = L.frames;
    if (IMIX) {
        const uint32_t pieces = s_off[w] >> 4;
        uint8_t *const dst0 = out + bytes0;
        for (uint32_t q0 = tid; q0 < pieces; q0 += 4 * BLOCK) {
            u32x4 v[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const uint32_t q = q0 + (uint32_t)u * BLOCK;
                if (q < pieces) {
                    const uint32_t b = q << 4;
                    uint32_t f = 0;   // the last frame below w that starts at or before byte b
#pragma unroll
                    for (uint32_t step = BLOCK / 2; step >= 1; step >>= 1)
                        if (f + step < w && s_off[f + step] <= b) f += step;
                    v[u] = __builtin_nontemporal_load(
                        (const u32x4 *)(pk + (unsigned long long)s_src[f] + (b - s_off[f])));
                }
            }
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const uint32_t q = q0 + (uint32_t)u * BLOCK;
                if (q < pieces) __builtin_nontemporal_store(v[u], (u32x4 *)(dst0 + ((unsigned long long)q << 4)));
            }
        }
    } else {
        const uint32_t P = L.copy_bytes >> 4;
        const uint32_t pieces = w * P;
        const bool pow2 = (P & (P - 1u)) == 0;
        const uint32_t sh = 31u - (uint32_t)__clz(P);
        const unsigned long long stride = L.h.stride, slot = L.slot_bytes;
        uint8_t *const dst0 = out + (unsigned long long)k0 * slot;
        for (uint32_t q0 = tid; q0 < pieces; q0 += 4 * BLOCK) {
            u32x4 v[4];
            uint32_t f[4], r[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const uint32_t q = q0 + (uint32_t)u * BLOCK;
                if (q < pieces) {
                    f[u] = pow2 ? q >> sh : q / P;
                    r[u] = (q - f[u] * P) << 4;
                    v[u] = __builtin_nontemporal_load((const u32x4 *)(pk + s_src[f[u]] * stride + r[u]));
                }
            }
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const uint32_t q = q0 + (uint32_t)u * BLOCK;
                if (q < pieces) __builtin_nontemporal_store(v[u], (u32x4 *)(dst0 + f[u] * slot + r[u]));
            }
        }
    }
}

}  // namespace

extern "C" hipError_t copk_tx_launch(const CopKTx *pp, int imix, hipStream_t stream)
{
    const CopKTx &p = *pp;
    if (!p.nl || !p.nchunks) return hipSuccess;
    if (p.nl > COPK_TX_MAXL || (imix && !p.sums)) return hipErrorInvalidValue;
    if (imix) {
        hipLaunchKernelGGL(cop_tx_sums, dim3(p.nchunks), dim3(BLOCK), 0, stream, p);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
        hipLaunchKernelGGL(cop_tx_copy<true>, dim3(p.nchunks), dim3(BLOCK), 0, stream, p);
    } else {
        hipLaunchKernelGGL(cop_tx_copy<false>, dim3(p.nchunks), dim3(BLOCK), 0, stream, p);
    }
    return hipGetLastError();
}
