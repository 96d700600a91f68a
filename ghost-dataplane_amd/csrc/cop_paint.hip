// cop_paint.hip — cop_lpm_paint: a whole DIR-24-8 image from sorted intervals.
//
// The image is a pure function of the table's (start, entry) intervals
// (lpm_build.c: fill_dir24 is that function with a running cursor). Here
// every entry finds its interval by a search instead:
//   tbl24[blk]       k = the last interval with starts[k] <= blk << 8; if the
//                    next interval starts inside the block, the block is
//                    extended and the entry is its rank in ext24 (the
//                    ascending list of extended blocks) | VALID_EXT, else
//                    entries[k]
//   tbl8[g*256 + a]  entries[last k with starts[k] <= (ext24[g] << 8) + a]
// The grid has two parts. Workgroups 0 .. 2^24 / COPK_PAINT_CHUNK - 1 each
// own COPK_PAINT_CHUNK consecutive blocks of tbl24; in the workgroups after
// them every wave owns one tbl8 group (groups n_ext .. cap_groups - 1 are
// zeroed). A workgroup (a wave, for a group) first finds the interval range
// [klo, khi] covering what it owns with two searches over all intervals whose
// operands are uniform, so they run on the scalar unit; its lanes then search
// inside that range only. Most chunks of a real table lie inside one or two
// intervals, so most lane searches take no step at all, and the range of a
// dense chunk (at most a few KiB of starts) is served by the vector L1 after
// the first touch: it is not staged in LDS, which keeps the kernel free of
// LDS and barriers and leaves the stores as the only thing that scales with
// the image.
// Stores: a lane writes four consecutive tbl24 entries as one 16-byte store,
// a wave 1 KiB contiguous, a workgroup 4 KiB per step; a tbl8 group is the
// same 1 KiB store of its wave. (One workgroup per group with a dword per lane
// measured 1.3x and 2.1x slower on the 100k- and 1M-route tables: DESIGN.md §22.5.)
// The kernel never runs beside a reader of the image: the runtime orders it
// between the launches of every lane (cop_runtime.cpp: live_replace).
#include <hip/hip_runtime.h>

#include "cop_kernels.h"

namespace {

constexpr uint32_t PAINT_BLOCK = 256;
constexpr uint32_t PAINT_CHUNKS = (1u << 24) / COPK_PAINT_CHUNK;
constexpr uint32_t PAINT_STEP = PAINT_BLOCK * 4;   // blocks per workgroup step
constexpr uint32_t PAINT_WAVES = PAINT_BLOCK / 64;  // tbl8 groups per workgroup: one per wave
constexpr uint32_t DIR_VALID_EXT = 0x03000000u;
static_assert(COPK_PAINT_CHUNK % PAINT_STEP == 0, "a chunk is whole steps");

// the last k in [lo, hi] with s[k] <= x (s[lo] <= x is given)
__device__ __forceinline__ uint32_t last_le(const uint32_t *__restrict__ s, uint32_t lo, uint32_t hi, uint32_t x)
{
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo + 1) / 2;
        if (s[mid] <= x) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// the first g in [lo, hi) with x[g] >= blk (hi if none)
__device__ __forceinline__ uint32_t rank_of(const uint32_t *__restrict__ x, uint32_t lo, uint32_t hi, uint32_t blk)
{
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (x[mid] < blk) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(PAINT_BLOCK) void cop_lpm_paint(const uint32_t *__restrict__ starts,
                                                             const uint32_t *__restrict__ entries, uint32_t niv,
                                                             const uint32_t *__restrict__ ext24, uint32_t n_ext,
                                                             uint32_t *__restrict__ tbl24, uint32_t *__restrict__ tbl8,
                                                             uint32_t cap_groups)
{
    const uint32_t wg = blockIdx.x, lane = threadIdx.x;
    if (wg >= PAINT_CHUNKS) {
        // one tbl8 group per wave: the group number is wave-uniform, so the
        // two searches for the block's interval range stay on the scalar unit
        const uint32_t g = __builtin_amdgcn_readfirstlane((wg - PAINT_CHUNKS) * PAINT_WAVES + lane / 64u);
        if (g >= cap_groups) return;
        const uint32_t a0 = (lane % 64u) * 4u;   // this lane's four entries of the group
        uint4 v = make_uint4(0, 0, 0, 0);
        if (g < n_ext) {
            const uint32_t lo = ext24[g] << 8;
            const uint32_t klo = last_le(starts, 0, niv - 1, lo);
            const uint32_t khi = last_le(starts, klo, niv - 1, lo | 255u);
            uint32_t k = last_le(starts, klo, khi, lo + a0);
            v.x = entries[k];
            k = last_le(starts, k, khi, lo + a0 + 1u);
            v.y = entries[k];
            k = last_le(starts, k, khi, lo + a0 + 2u);
            v.z = entries[k];
            k = last_le(starts, k, khi, lo + a0 + 3u);
            v.w = entries[k];
        }
        *reinterpret_cast<uint4 *>(tbl8 + (size_t)g * 256 + a0) = v;
        return;
    }
    const uint32_t b0 = wg * COPK_PAINT_CHUNK, b1 = b0 + COPK_PAINT_CHUNK - 1;
    const uint32_t klo = last_le(starts, 0, niv - 1, b0 << 8);
    const uint32_t khi = last_le(starts, klo, niv - 1, (b1 << 8) | 255u);
    if (klo == khi) {
        // the whole chunk lies inside one interval
        const uint32_t e = entries[klo];
        const uint4 e4 = make_uint4(e, e, e, e);
        for (uint32_t q = b0 + lane * 4u; q <= b1; q += PAINT_STEP) *reinterpret_cast<uint4 *>(tbl24 + q) = e4;
        return;
    }
    const uint32_t glo = rank_of(ext24, 0, n_ext, b0);
    const uint32_t ghi = rank_of(ext24, glo, n_ext, b1 + 1);
    for (uint32_t q = b0 + lane * 4u; q <= b1; q += PAINT_STEP) {
        uint32_t v[4];
        uint32_t k = klo;
#pragma unroll
        for (uint32_t i = 0; i < 4; i++) {
            const uint32_t blk = q + i;
            k = last_le(starts, k, khi, blk << 8);   // blocks ascend: the search starts at the last one's interval
            if (k < khi && starts[k + 1] <= ((blk << 8) | 255u)) v[i] = rank_of(ext24, glo, ghi, blk) | DIR_VALID_EXT;
            else v[i] = entries[k];
        }
        *reinterpret_cast<uint4 *>(tbl24 + q) = make_uint4(v[0], v[1], v[2], v[3]);
    }
}

}  // namespace

extern "C" hipError_t copk_paint_launch(const uint32_t *starts, const uint32_t *entries, uint32_t niv,
                                        const uint32_t *ext24, uint32_t n_ext, uint32_t *tbl24, uint32_t *tbl8,
                                        uint32_t cap_groups, hipStream_t stream)
{
    // starts[0] == 0 is the caller's to check: the arrays are device memory
    if (!starts || !entries || !tbl24 || niv == 0 || n_ext > cap_groups || cap_groups > (1u << 24)) return hipErrorInvalidValue;
    if ((n_ext && !ext24) || (cap_groups && !tbl8)) return hipErrorInvalidValue;
    if (((uintptr_t)tbl24 | (uintptr_t)tbl8) & 15u) return hipErrorInvalidValue;
    if (((uintptr_t)starts | (uintptr_t)entries | (uintptr_t)ext24) & 3u) return hipErrorInvalidValue;
    hipLaunchKernelGGL(cop_lpm_paint, dim3(PAINT_CHUNKS + (cap_groups + PAINT_WAVES - 1) / PAINT_WAVES), dim3(PAINT_BLOCK), 0, stream, starts, entries, niv,
                       ext24, n_ext, tbl24, tbl8, cap_groups);
    return hipGetLastError();
}
