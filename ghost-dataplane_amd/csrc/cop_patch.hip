// cop_patch.hip — cop_lpm_patch: apply fill records to a DIR-24-8 image.
//
// A table update arrives as disjoint records {table, first, count, entry}:
// entries [first, first + count) of tbl24 (table 0) or tbl8 (table 1) become
// `entry` (lpm_live.c: cop_lpm_patch_records). Updates come in two shapes
// and the kernel has one path for both: a burst of thousands of one-entry
// records (host routes), and single runs of up to 2^23 entries (a /1: 32 MiB
// of tbl24). The host cuts long runs into records of at most COPK_PATCH_SPAN
// entries, so a long run is shared by many workgroups, and every record gets
// PATCH_LANES = 16 lanes, a quarter wave: a one-entry record idles 15 lanes,
// not a workgroup, and a full record's lanes write 256 contiguous bytes per
// step. The kernel is correct for any count; the cut only spreads the work.
//
// Per record: the head up to the first 16-byte boundary and the tail after
// the last one go out as dword stores (at most 3 each), the aligned body as
// 16-byte vector stores. Records are disjoint, so no two lanes of the launch
// write the same word and no ordering between them is needed. The kernel
// never runs beside a reader of the image: the runtime orders it between the
// launches of every lane (cop_runtime.cpp: live_apply).
#include <hip/hip_runtime.h>

#include "cop_kernels.h"

namespace {

constexpr uint32_t PATCH_BLOCK = 256;
constexpr uint32_t PATCH_LANES = 16;   // lanes per record

__global__ __launch_bounds__(PATCH_BLOCK) void cop_lpm_patch(const uint4 *__restrict__ recs, uint32_t n,
                                                             uint32_t *__restrict__ tbl24, uint32_t cap24,
                                                             uint32_t *__restrict__ tbl8, uint32_t cap8)
{
    const uint32_t gid = blockIdx.x * PATCH_BLOCK + threadIdx.x;
    const uint32_t r = gid / PATCH_LANES, lane = gid % PATCH_LANES;
    if (r >= n) return;
    const uint4 rec = recs[r];   // the record's 16 lanes read the same 16 bytes
    uint32_t *base = rec.x ? tbl8 : tbl24;
    const uint32_t cap = rec.x ? cap8 : cap24;
    const uint32_t first = rec.y, count = rec.z, e = rec.w;
    // a record that leaves its table is dropped whole (the host checks too)
    if (rec.x > 1u || first > cap || count > cap - first) return;
    const uint32_t end = first + count;
    const uint32_t head_end = min(end, (first + 3u) & ~3u);   // first 4-entry boundary, or the run's end
    const uint32_t body_end = max(head_end, end & ~3u);
    if (first + lane < head_end) base[first + lane] = e;
    const uint4 e4 = make_uint4(e, e, e, e);
    for (uint32_t q = head_end + lane * 4u; q < body_end; q += PATCH_LANES * 4u)
        *reinterpret_cast<uint4 *>(base + q) = e4;
    if (body_end + lane < end) base[body_end + lane] = e;
}

}  // namespace

extern "C" hipError_t copk_patch_launch(const void *recs, uint32_t n, uint32_t *tbl24, uint32_t cap24, uint32_t *tbl8,
                                        uint32_t cap8, hipStream_t stream)
{
    if (!n) return hipSuccess;
    // n <= 2^24 records keeps gid inside 32 bits
    if (n > (1u << 24) || ((uintptr_t)tbl24 | (uintptr_t)tbl8 | (uintptr_t)recs) & 15u) return hipErrorInvalidValue;
    const uint32_t grid = (uint32_t)(((uint64_t)n * PATCH_LANES + PATCH_BLOCK - 1) / PATCH_BLOCK);
    hipLaunchKernelGGL(cop_lpm_patch, dim3(grid), dim3(PATCH_BLOCK), 0, stream, (const uint4 *)recs, n, tbl24, cap24,
                       tbl8, cap8);
    return hipGetLastError();
}
