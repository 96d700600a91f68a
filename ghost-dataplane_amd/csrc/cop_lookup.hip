// cop_lookup.hip — cop_lpm_lookup: rte_lpm_lookup_bulk over a stage's device
// table (cop_lookup_bulk, include/cop_gpu.h).
//
// A stream of u32 addresses in, one word per address out; nothing else: no
// frames, no verdicts, no counters, no forward list. The lookups are the
// pipeline's own (cop_device.h: ivt_value, probe_ld + tbl8_step, trie_walk,
// bkt_issue + bkt_step), so every table form the pipeline reads is read here
// the same way.
//
// Tile: 256 lanes x APL addresses (APL 8; 4 in the bucketed form, whose
// second round holds four 16-byte registers per address, as the pipeline's
// tile size for it). VEC (both pointers 16-byte aligned): lane t moves the 4
// consecutive addresses at tile + (j * 256 + t) * 4, j < APL / 4, as one
// 16-byte access, so a wave instruction covers 1 KiB of contiguous addresses;
// the group that straddles n falls back to dword accesses for its valid
// elements. Without VEC lane t handles addresses j * 256 + t by dword
// accesses, 256 contiguous bytes per wave instruction. Loads and stores are
// non-temporal: an address is read once and a word is never read back.
// Nothing at index >= n is read or written; lanes past the end look address
// 0 up (always inside every table) with live = false and store nothing.
//
// A lane's APL first-round loads (tbl24 probes, bucket index, trie nodes) are
// all issued before any second-round load, as inside tbl8_step, trie_walk and
// bkt_step. The LDS forms stage their image (interval starts + u16 bucket
// index + values, up to about 72 KiB: 2 workgroups per CU; the trie's 4096
// top entries) once per workgroup by LDS-DMA, first thing, and the grid is a
// grid-stride loop over tiles sized to the resident workgroups, so the
// staging is paid once per workgroup, not per tile.
//
// In place (out == ips) is safe: a lane writes exactly the elements it read,
// after it read them, and no other lane touches them.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "cop_device.h"
#include "cop_kernels.h"

namespace {

using namespace copd;

template <int FORM, int APL, bool VEC>
__global__ __launch_bounds__(BLOCK) void cop_lpm_lookup(const CopKLookup p)
{
    static_assert(APL % 4 == 0, "16-byte groups");
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    constexpr uint32_t TILE = BLOCK * APL;

    // LDS carve: starts + index (m + iw words, both multiples of 4) | values
    uint32_t *const S = lds;
    uint32_t *const V = lds + p.m + p.iw;
    const StageSeg none{nullptr, nullptr, 0u};
    if (FORM == COPK_TBL_IVT)
        lds_stage_all(StageSeg{p.starts, S, (p.m + p.iw) >> 2}, StageSeg{p.vals, V, p.m >> 2}, none, none, none, none,
                      lane, wave);
    if (FORM == COPK_TBL_TRIE)
        lds_stage_all(StageSeg{p.tl0, lds, COPK_TRIE_L0 / 4u}, none, none, none, none, none, lane, wave);
    bool staged = !(FORM == COPK_TBL_IVT || FORM == COPK_TBL_TRIE);

    for (uint32_t tile = blockIdx.x; tile < p.ntiles; tile += gridDim.x) {
        const uint32_t base = tile * TILE;    // < n
        const uint32_t rem = p.n - base;      // addresses from base on (>= 1)
        const uint32_t *const in = p.ips + base;
        uint32_t *const out = p.out + base;

        uint32_t ip[APL];
        bool live[APL];
        if (VEC) {
#pragma unroll
            for (int j = 0; j < APL / 4; j++) {
                const uint32_t off = ((uint32_t)j * BLOCK + (uint32_t)tid) * 4u;
                if (off + 4u <= rem) {
                    const u32x4 v = __builtin_nontemporal_load((const u32x4 *)(in + off));
                    ip[4 * j + 0] = v.x;
                    ip[4 * j + 1] = v.y;
                    ip[4 * j + 2] = v.z;
                    ip[4 * j + 3] = v.w;
#pragma unroll
                    for (int q = 0; q < 4; q++) live[4 * j + q] = true;
                } else {
#pragma unroll
                    for (int q = 0; q < 4; q++) {
                        live[4 * j + q] = off + (uint32_t)q < rem;
                        ip[4 * j + q] = live[4 * j + q] ? __builtin_nontemporal_load(in + off + q) : 0u;
                    }
                }
            }
        } else {
#pragma unroll
            for (int k = 0; k < APL; k++) {
                const uint32_t idx = (uint32_t)k * BLOCK + (uint32_t)tid;
                live[k] = idx < rem;
                ip[k] = live[k] ? __builtin_nontemporal_load(in + idx) : 0u;
            }
        }
        if (!staged) {   // workgroup-uniform: the first tile waits for the LDS-DMA staging (counted by vmcnt)
            __syncthreads();
            staged = true;
        }

        uint32_t e[APL];
        if (FORM == COPK_TBL_IVT) {
#pragma unroll
            for (int k = 0; k < APL; k++) e[k] = ivt_value(S, V, p.m, p.ib, p.lv, ip[k]);
        }
        if (FORM == COPK_TBL_DIR) {
#pragma unroll
            for (int k = 0; k < APL; k++) e[k] = probe_ld(&p.tbl24[ip[k] >> 8], p.probe_nt);
            tbl8_step<APL>(p.tbl8, p.tbl8_packed, ip, e);
        }
        if (FORM == COPK_TBL_TRIE) {
#pragma unroll
            for (int k = 0; k < APL; k++) e[k] = lds[ip[k] >> 20];
            trie_walk<APL>(p.tnodes, p.tleaves, ip, e, live);
        }
        if (FORM == COPK_TBL_BKT) {
            uint32_t k1[APL];
#pragma unroll
            for (int k = 0; k < APL; k++) bkt_issue(p.bidx, p.ib, ip[k], live[k], e[k], k1[k]);
            bkt_step<APL>(p.bpairs, ip, e, k1, live);
        }
        // the public word: the entry without its depth / valid_group bits, 0 on a miss
#pragma unroll
        for (int k = 0; k < APL; k++) e[k] = (e[k] & COPK_LOOKUP_HIT) ? (e[k] & p.mask) : 0u;

        if (VEC) {
#pragma unroll
            for (int j = 0; j < APL / 4; j++) {
                const uint32_t off = ((uint32_t)j * BLOCK + (uint32_t)tid) * 4u;
                if (off + 4u <= rem) {
                    __builtin_nontemporal_store(u32x4{e[4 * j], e[4 * j + 1], e[4 * j + 2], e[4 * j + 3]},
                                                (u32x4 *)(out + off));
                } else {
#pragma unroll
                    for (int q = 0; q < 4; q++)
                        if (live[4 * j + q]) __builtin_nontemporal_store(e[4 * j + q], out + off + q);
                }
            }
        } else {
#pragma unroll
            for (int k = 0; k < APL; k++)
                if (live[k]) __builtin_nontemporal_store(e[k], out + (uint32_t)k * BLOCK + (uint32_t)tid);
        }
    }
}

template <int FORM, int APL, bool VEC>
hipError_t lookup_one(const CopKLookup &p, uint32_t lds_bytes, uint32_t ncu, uint32_t grid_cap, hipStream_t s)
{
    // as many workgroups as stay resident, each looping over its share of the tiles
    int per_cu = 0;
    hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, cop_lpm_lookup<FORM, APL, VEC>, BLOCK, lds_bytes);
    if (e != hipSuccess) return e;
    if (per_cu < 1) return hipErrorInvalidConfiguration;
    uint32_t grid = (uint32_t)std::min<uint64_t>(p.ntiles, (uint64_t)ncu * (uint32_t)per_cu);
    if (grid_cap) grid = std::min(grid, grid_cap);
    hipLaunchKernelGGL((cop_lpm_lookup<FORM, APL, VEC>), dim3(grid), dim3(BLOCK), lds_bytes, s, p);
    return hipGetLastError();
}

template <int FORM, int APL>
hipError_t lookup_form(CopKLookup &p, uint32_t lds_bytes, uint32_t ncu, uint32_t grid_cap, hipStream_t s)
{
    constexpr uint32_t TILE = BLOCK * APL;
    p.ntiles = (uint32_t)(((uint64_t)p.n + TILE - 1) / TILE);
    const bool vec = (((uintptr_t)p.ips | (uintptr_t)p.out) & 15u) == 0;
    return vec ? lookup_one<FORM, APL, true>(p, lds_bytes, ncu, grid_cap, s)
               : lookup_one<FORM, APL, false>(p, lds_bytes, ncu, grid_cap, s);
}

}  // namespace

extern "C" hipError_t copk_lookup_launch(const CopKLookup *pp, int form, uint32_t ncu, uint32_t grid_cap,
                                         hipStream_t stream)
{
    CopKLookup p = *pp;
    if (!p.n) return hipSuccess;
    if (!p.ips || !p.out || (((uintptr_t)p.ips | (uintptr_t)p.out) & 3u)) return hipErrorInvalidValue;
    switch (form) {
    case COPK_TBL_IVT:
        if (!p.starts || !p.vals || p.m < 4u || (p.m & 3u) || (p.iw & 3u)) return hipErrorInvalidValue;
        return lookup_form<COPK_TBL_IVT, 8>(p, (2u * p.m + p.iw) * 4u, ncu, grid_cap, stream);
    case COPK_TBL_DIR:
        if (!p.tbl24 || !p.tbl8) return hipErrorInvalidValue;
        return lookup_form<COPK_TBL_DIR, 8>(p, 0u, ncu, grid_cap, stream);
    case COPK_TBL_TRIE:
        if (!p.tl0 || !p.tnodes || !p.tleaves) return hipErrorInvalidValue;
        return lookup_form<COPK_TBL_TRIE, 8>(p, COPK_TRIE_L0 * 4u, ncu, grid_cap, stream);
    case COPK_TBL_BKT:
        if (!p.bidx || !p.bpairs) return hipErrorInvalidValue;
        return lookup_form<COPK_TBL_BKT, 4>(p, 0u, ncu, grid_cap, stream);
    default:
        return hipErrorInvalidValue;
    }
}
