// cop_aead.hip — cop_aead_xor / cop_aead_mac / cop_aead_status: ChaCha20-Poly1305
// (RFC 8439) over the frames of tx bursts in device memory (cop_aead_seal /
// cop_aead_open / cop_poly1305_bulk, include/cop_gpu.h "AEAD"; host mirror:
// aead.c). Three kernels, separate launches for separate phases, no atomics and
// no workgroup waiting for another:
//
// Keystream (cop_aead_xor): `group` lanes per frame (a power of two the host
// picks per burst: enough for every 64-byte region of a slot frame, 8 for
// off / len bursts, whose lanes loop). The text starts at byte a of the frame,
// the frame's 16-byte pieces at byte 0, so keystream and pieces are out of
// step by s = a & 15 bytes. A lane owns the 64 frame bytes [a0 + 64 j, + 64)
// (a0 = a & ~15): it computes ChaCha block j (counter j + 1) in 16 VGPRs, takes
// the last 16 keystream bytes of block j - 1 from the lane below it (four
// shuffles; lane 0 of a group from the group's last lane of the previous
// round), cuts its 64 bytes out of the 80 at byte 16 - s (whole words by a
// switch over compile-time offsets, so nothing is indexed at run time and
// nothing goes to scratch; the odd bytes by v_alignbyte), and
// XORs its four pieces with 16-byte loads and stores. Bytes outside [a, l) are
// masked out of the keystream, so the read-modify-write gives them back as
// they were; no two lanes share a piece. Open passes ok[]: a frame whose word
// is not 1 is left alone.
//
// MAC (cop_aead_mac): one frame per lane. The one-time key is ChaCha block 0
// (or otk[k] for cop_poly1305_bulk); Poly1305 runs in five 26-bit limbs with
// 32 x 32 -> 64 products (aead.c's code) over AD || pad16 || text || pad16 ||
// lengths, the text blocks cut from two neighbouring pieces at a time. Seal
// writes the tag, open compares it with tags[k] and writes ok[k].
//
// Status (cop_aead_status): every wave of the MAC kernel leaves its counts
// (processed, tag failures, skipped) in context-owned scratch, one 16-byte
// record per wave; one workgroup per burst sums the burst's records and writes
// the four status words.
//
// Only vector loads and stores, in plain C++ and __builtin_*.
//
// Bounds: frame k is touched only if k < min(*count, n_frames), off is a
// multiple of 16 and off + ext <= cap_bytes (ext = (l + 15) & ~15, l <= 2048);
// every piece loaded or stored starts at a multiple of 16 below ext, so it
// lies inside the frame's [0, ext); tags / ok / otk are indexed by that k.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cop_chunk.h"   // item_of, wave_sum

namespace {

constexpr int BLOCK = COPK_AE_BLOCK;

__device__ __forceinline__ uint32_t frames_present(const CopKAeBurst &B)
{
    return B.count ? min(*B.count, B.n_frames) : B.n_frames;
}

// frame k (below frames_present): true and (o, l) if it is processed, false if skipped
__device__ __forceinline__ bool frame_of(const CopKAeBurst &B, uint32_t k, uint32_t &o, uint32_t &l)
{
    l = B.off ? min(B.len[k], COPK_TX_MAX_FRAME) : B.frame_bytes;
    const unsigned long long off = B.off ? (unsigned long long)B.off[k] : (unsigned long long)k * B.slot_bytes;
    o = (uint32_t)off;
    return !(off & 15ull) && off + ((l + 15u) & ~15u) <= (unsigned long long)B.cap_bytes;
}

#define COP_QR(a, b, c, d)                                 \
    do {                                                   \
        a += b, d ^= a, d = __builtin_rotateleft32(d, 16); \
        c += d, b ^= c, b = __builtin_rotateleft32(b, 12); \
        a += b, d ^= a, d = __builtin_rotateleft32(d, 8);  \
        c += d, b ^= c, b = __builtin_rotateleft32(b, 7);  \
    } while (0)

// one ChaCha20 block: x[16] in VGPRs
__device__ __forceinline__ void chacha_block(const CopKAead &p, uint32_t counter, unsigned long long seq, uint32_t x[16])
{
    uint32_t s[16];
    s[0] = 0x61707865u, s[1] = 0x3320646eu, s[2] = 0x79622d32u, s[3] = 0x6b206574u;
#pragma unroll
    for (int i = 0; i < 8; i++) s[4 + i] = p.key[i];
    s[12] = counter, s[13] = p.salt, s[14] = (uint32_t)seq, s[15] = (uint32_t)(seq >> 32);
#pragma unroll
    for (int i = 0; i < 16; i++) x[i] = s[i];
#pragma unroll
    for (int r = 0; r < 10; r++) {
        COP_QR(x[0], x[4], x[8], x[12]);
        COP_QR(x[1], x[5], x[9], x[13]);
        COP_QR(x[2], x[6], x[10], x[14]);
        COP_QR(x[3], x[7], x[11], x[15]);
        COP_QR(x[0], x[5], x[10], x[15]);
        COP_QR(x[1], x[6], x[11], x[12]);
        COP_QR(x[2], x[7], x[8], x[13]);
        COP_QR(x[3], x[4], x[9], x[14]);
    }
#pragma unroll
    for (int i = 0; i < 16; i++) x[i] += s[i];
}

// the bytes of the word at frame position pos that lie in [lo, hi), as a mask
__device__ __forceinline__ uint32_t byte_mask(uint32_t pos, uint32_t lo, uint32_t hi)
{
    const int b0 = max((int)lo - (int)pos, 0), b1 = min((int)hi - (int)pos, 4);
    return b1 > b0 ? (0xFFFFFFFFu >> (8 * (4 - b1))) & (0xFFFFFFFFu << (8 * b0)) : 0u;   // shifts of 0..24
}

// One lane's 64-byte region at frame position pos (a multiple of 16): K = prev (16 bytes) || ks (64
// bytes), the region's keystream byte b is K[4 WS + bs + b]. The pieces that start below l are XORed
// with the keystream bytes that fall in [a, l); pos < l puts a piece below ext.
template <int WS>
__device__ __forceinline__ void xor_region(const uint32_t (&prev)[4], const uint32_t (&ks)[16], uint32_t bs, uint8_t *at,
                                           uint32_t pos, uint32_t a, uint32_t l)
{
    uint32_t K[22];
#pragma unroll
    for (int i = 0; i < 4; i++) K[i] = prev[i];
#pragma unroll
    for (int i = 0; i < 16; i++) K[4 + i] = ks[i];
    K[20] = K[21] = 0u;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        if (pos + 16u * q < l) {
            u32x4 w;
            w.x = __builtin_amdgcn_alignbyte(K[WS + 4 * q + 1], K[WS + 4 * q + 0], bs) & byte_mask(pos + 16u * q, a, l);
            w.y = __builtin_amdgcn_alignbyte(K[WS + 4 * q + 2], K[WS + 4 * q + 1], bs) & byte_mask(pos + 16u * q + 4u, a, l);
            w.z = __builtin_amdgcn_alignbyte(K[WS + 4 * q + 3], K[WS + 4 * q + 2], bs) & byte_mask(pos + 16u * q + 8u, a, l);
            w.w = __builtin_amdgcn_alignbyte(K[WS + 4 * q + 4], K[WS + 4 * q + 3], bs) & byte_mask(pos + 16u * q + 12u, a, l);
            u32x4 *const piece = (u32x4 *)(at + 16 * q);
            *piece = *piece ^ w;
        }
    }
}

__global__ __launch_bounds__(BLOCK) void cop_aead_xor(const CopKAead p)
{
    const CopKAeBurst &B = p.b[item_of(p.nb, blockIdx.x, [&](uint32_t i) { return p.b[i].xor_begin; })];
    const uint32_t G = B.group, tid = threadIdx.x;
    const uint32_t j = tid & (G - 1u), g = tid / G;
    const uint32_t k = (blockIdx.x - B.xor_begin) * (BLOCK / G) + g;
    uint32_t o = 0, l = 0, a = 0;
    bool live = k < frames_present(B);
    if (live) live = frame_of(B, k, o, l);
    if (live && B.ok) live = B.ok[k] == 1u;
    if (live) a = min(B.aad_bytes, l);
    const uint32_t T = live ? l - a : 0u, a0 = a & ~15u;
    const uint32_t R = T ? (l - a0 + 63u) / 64u : 0u;   // 64-byte regions that hold text: <= 32
    const uint32_t t = 16u - (a & 15u);                           // keystream byte b of a region is K[t + b]
    uint8_t *const f = B.frames + o;
    const unsigned long long seq = B.seq_base + k;

    uint32_t carry[4] = {0u, 0u, 0u, 0u};
    for (uint32_t it = 0; __any(it * G < R); it++) {
        const uint32_t blk = it * G + j;
        uint32_t ks[16];
#pragma unroll
        for (int i = 0; i < 16; i++) ks[i] = 0u;
        if (blk * 64u < T) chacha_block(p, blk + 1u, seq, ks);   // T == 0 where not live
        // the last 16 bytes of block blk - 1
        uint32_t prev[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const uint32_t below = (uint32_t)__shfl_up((int)ks[12 + i], 1, (int)G);
            const uint32_t wrap = (uint32_t)__shfl((int)carry[i], (int)(G - 1u), (int)G);
            prev[i] = j ? below : wrap;
        }
#pragma unroll
        for (int i = 0; i < 4; i++) carry[i] = ks[12 + i];
        if (blk < R) {
            // down by t = 1..16 bytes: whole words by the case, the rest by v_alignbyte
            uint8_t *const at = f + a0 + 64u * blk;
            const uint32_t pos = a0 + 64u * blk;
            switch (t >> 2) {
            case 0: xor_region<0>(prev, ks, t & 3u, at, pos, a, l); break;
            case 1: xor_region<1>(prev, ks, t & 3u, at, pos, a, l); break;
            case 2: xor_region<2>(prev, ks, t & 3u, at, pos, a, l); break;
            case 3: xor_region<3>(prev, ks, t & 3u, at, pos, a, l); break;
            default: xor_region<4>(prev, ks, 0u, at, pos, a, l); break;
            }
        }
    }
}

// ---- Poly1305, 26-bit limbs (aead.c's arithmetic) ---------------------------------
struct Poly {
    uint32_t r0, r1, r2, r3, r4, h0, h1, h2, h3, h4;
};

__device__ __forceinline__ void poly_init(Poly &P, uint32_t t0, uint32_t t1, uint32_t t2, uint32_t t3)
{
    P.r0 = t0 & 0x3ffffffu;
    P.r1 = ((t0 >> 26) | (t1 << 6)) & 0x3ffff03u;
    P.r2 = ((t1 >> 20) | (t2 << 12)) & 0x3ffc0ffu;
    P.r3 = ((t2 >> 14) | (t3 << 18)) & 0x3f03fffu;
    P.r4 = (t3 >> 8) & 0x00fffffu;
    P.h0 = P.h1 = P.h2 = P.h3 = P.h4 = 0u;
}

__device__ __forceinline__ void poly_block(Poly &P, u32x4 m, uint32_t hibit)
{
    typedef unsigned long long u64;
    const uint32_t r0 = P.r0, r1 = P.r1, r2 = P.r2, r3 = P.r3, r4 = P.r4;
    const uint32_t s1 = r1 * 5u, s2 = r2 * 5u, s3 = r3 * 5u, s4 = r4 * 5u;
    uint32_t h0 = P.h0, h1 = P.h1, h2 = P.h2, h3 = P.h3, h4 = P.h4, c;
    h0 += m.x & 0x3ffffffu;
    h1 += ((m.x >> 26) | (m.y << 6)) & 0x3ffffffu;
    h2 += ((m.y >> 20) | (m.z << 12)) & 0x3ffffffu;
    h3 += ((m.z >> 14) | (m.w << 18)) & 0x3ffffffu;
    h4 += (m.w >> 8) | hibit;
    u64 d0 = (u64)h0 * r0 + (u64)h1 * s4 + (u64)h2 * s3 + (u64)h3 * s2 + (u64)h4 * s1;
    u64 d1 = (u64)h0 * r1 + (u64)h1 * r0 + (u64)h2 * s4 + (u64)h3 * s3 + (u64)h4 * s2;
    u64 d2 = (u64)h0 * r2 + (u64)h1 * r1 + (u64)h2 * r0 + (u64)h3 * s4 + (u64)h4 * s3;
    u64 d3 = (u64)h0 * r3 + (u64)h1 * r2 + (u64)h2 * r1 + (u64)h3 * r0 + (u64)h4 * s4;
    u64 d4 = (u64)h0 * r4 + (u64)h1 * r3 + (u64)h2 * r2 + (u64)h3 * r1 + (u64)h4 * r0;
    c = (uint32_t)(d0 >> 26), h0 = (uint32_t)d0 & 0x3ffffffu, d1 += c;
    c = (uint32_t)(d1 >> 26), h1 = (uint32_t)d1 & 0x3ffffffu, d2 += c;
    c = (uint32_t)(d2 >> 26), h2 = (uint32_t)d2 & 0x3ffffffu, d3 += c;
    c = (uint32_t)(d3 >> 26), h3 = (uint32_t)d3 & 0x3ffffffu, d4 += c;
    c = (uint32_t)(d4 >> 26), h4 = (uint32_t)d4 & 0x3ffffffu, h0 += c * 5u;
    c = h0 >> 26, h0 &= 0x3ffffffu, h1 += c;
    P.h0 = h0, P.h1 = h1, P.h2 = h2, P.h3 = h3, P.h4 = h4;
}

__device__ __forceinline__ u32x4 poly_finish(const Poly &P, uint32_t p0, uint32_t p1, uint32_t p2, uint32_t p3)
{
    typedef unsigned long long u64;
    uint32_t h0 = P.h0, h1 = P.h1, h2 = P.h2, h3 = P.h3, h4 = P.h4, c;
    c = h1 >> 26, h1 &= 0x3ffffffu, h2 += c;
    c = h2 >> 26, h2 &= 0x3ffffffu, h3 += c;
    c = h3 >> 26, h3 &= 0x3ffffffu, h4 += c;
    c = h4 >> 26, h4 &= 0x3ffffffu, h0 += c * 5u;
    c = h0 >> 26, h0 &= 0x3ffffffu, h1 += c;
    uint32_t g0 = h0 + 5u, g1, g2, g3, g4;
    c = g0 >> 26, g0 &= 0x3ffffffu;
    g1 = h1 + c, c = g1 >> 26, g1 &= 0x3ffffffu;
    g2 = h2 + c, c = g2 >> 26, g2 &= 0x3ffffffu;
    g3 = h3 + c, c = g3 >> 26, g3 &= 0x3ffffffu;
    g4 = h4 + c - (1u << 26);
    const bool take_g = !(g4 >> 31);   // h >= 2^130 - 5
    h0 = take_g ? g0 : h0, h1 = take_g ? g1 : h1, h2 = take_g ? g2 : h2, h3 = take_g ? g3 : h3, h4 = take_g ? g4 : h4;
    const uint32_t w0 = h0 | (h1 << 26), w1 = (h1 >> 6) | (h2 << 20), w2 = (h2 >> 12) | (h3 << 14),
                   w3 = (h3 >> 18) | (h4 << 8);
    u32x4 tag;
    u64 fsum = (u64)w0 + p0;
    tag.x = (uint32_t)fsum;
    fsum = (u64)w1 + p1 + (fsum >> 32);
    tag.y = (uint32_t)fsum;
    fsum = (u64)w2 + p2 + (fsum >> 32);
    tag.z = (uint32_t)fsum;
    fsum = (u64)w3 + p3 + (fsum >> 32);
    tag.w = (uint32_t)fsum;
    return tag;
}

// keeps the first n (0..16) bytes of a block
__device__ __forceinline__ u32x4 keep_bytes(u32x4 v, uint32_t n)
{
    v.x &= byte_mask(0u, 0u, n), v.y &= byte_mask(4u, 0u, n), v.z &= byte_mask(8u, 0u, n), v.w &= byte_mask(12u, 0u, n);
    return v;
}

// the 16 bytes that start 4 WS + bs bytes into cur || nxt
template <int WS>
__device__ __forceinline__ u32x4 cut(u32x4 cur, u32x4 nxt, uint32_t bs)
{
    const uint32_t M[9] = {cur.x, cur.y, cur.z, cur.w, nxt.x, nxt.y, nxt.z, nxt.w, 0u};
    u32x4 m;
    m.x = __builtin_amdgcn_alignbyte(M[WS + 1], M[WS + 0], bs);
    m.y = __builtin_amdgcn_alignbyte(M[WS + 2], M[WS + 1], bs);
    m.z = __builtin_amdgcn_alignbyte(M[WS + 3], M[WS + 2], bs);
    m.w = __builtin_amdgcn_alignbyte(M[WS + 4], M[WS + 3], bs);
    return m;
}

// frame bytes [from, to) as pad16 blocks; from and to - from arbitrary, every piece read lies below ext
__device__ __forceinline__ void poly_span(Poly &P, const uint8_t *f, uint32_t ext, uint32_t from, uint32_t to)
{
    if (to <= from) return;
    const uint32_t sh = from & 15u, ws = sh >> 2, bs = sh & 3u;
    uint32_t q = from & ~15u;
    u32x4 cur = *(const u32x4 *)(f + q);
    for (uint32_t pos = from; pos < to; pos += 16u, q += 16u) {
        u32x4 nxt = u32x4{0u, 0u, 0u, 0u};
        if (q + 16u < ext && q + 16u < to) nxt = *(const u32x4 *)(f + q + 16u);
        u32x4 m;
        switch (ws) {
        case 0: m = cut<0>(cur, nxt, bs); break;
        case 1: m = cut<1>(cur, nxt, bs); break;
        case 2: m = cut<2>(cur, nxt, bs); break;
        default: m = cut<3>(cur, nxt, bs); break;
        }
        if (to - pos < 16u) m = keep_bytes(m, to - pos);
        poly_block(P, m, 1u << 24);
        cur = nxt;
    }
}

__global__ __launch_bounds__(BLOCK) void cop_aead_mac(const CopKAead p)
{
    const CopKAeBurst &B = p.b[item_of(p.nb, blockIdx.x, [&](uint32_t i) { return p.b[i].mac_begin; })];
    const uint32_t k = (blockIdx.x - B.mac_begin) * BLOCK + threadIdx.x;
    const bool present = k < frames_present(B);
    uint32_t o = 0, l = 0;
    const bool live = present && frame_of(B, k, o, l);
    bool bad = false;
    if (live) {
        const uint8_t *const f = B.frames + o;
        const uint32_t ext = (l + 15u) & ~15u;
        Poly P;
        uint32_t pad[4];
        if (p.mode == COPK_AE_POLY) {
            const uint32_t *const kw = (const uint32_t *)(B.otk + 32ull * k);
            poly_init(P, kw[0], kw[1], kw[2], kw[3]);
            pad[0] = kw[4], pad[1] = kw[5], pad[2] = kw[6], pad[3] = kw[7];
            uint32_t pos = 0;
            for (; pos + 16u <= l; pos += 16u) poly_block(P, *(const u32x4 *)(f + pos), 1u << 24);
            if (pos < l) {   // the final 1..15 bytes, a 1 after them and no high bit
                const uint32_t n = l - pos;
                u32x4 m = keep_bytes(*(const u32x4 *)(f + pos), n);
                const uint32_t one = 1u << (8u * (n & 3u));
                m.x |= (n >> 2) == 0u ? one : 0u, m.y |= (n >> 2) == 1u ? one : 0u;
                m.z |= (n >> 2) == 2u ? one : 0u, m.w |= (n >> 2) == 3u ? one : 0u;
                poly_block(P, m, 0u);
            }
        } else {
            uint32_t x[16];
            chacha_block(p, 0u, B.seq_base + k, x);
            poly_init(P, x[0], x[1], x[2], x[3]);
            pad[0] = x[4], pad[1] = x[5], pad[2] = x[6], pad[3] = x[7];
            const uint32_t a = min(B.aad_bytes, l);
            poly_span(P, f, ext, 0u, a);
            poly_span(P, f, ext, a, l);
            poly_block(P, u32x4{a, 0u, l - a, 0u}, 1u << 24);
        }
        const u32x4 tag = poly_finish(P, pad[0], pad[1], pad[2], pad[3]);
        u32x4 *const slot = (u32x4 *)(B.tags + 16ull * k);
        if (p.mode == COPK_AE_OPEN) {
            const u32x4 want = *slot;
            bad = ((tag.x ^ want.x) | (tag.y ^ want.y) | (tag.z ^ want.z) | (tag.w ^ want.w)) != 0u;
            B.ok[k] = bad ? 0u : 1u;
        } else {
            *slot = tag;
        }
    }
    // the wave's counts for cop_aead_status: every lane arrives here
    const uint32_t n_present = (uint32_t)__popcll(__ballot(present)), n_live = (uint32_t)__popcll(__ballot(live)),
                   n_bad = (uint32_t)__popcll(__ballot(bad));
    if ((threadIdx.x & 63u) == 0u)
        ((u32x4 *)p.scratch)[(size_t)(p.scratch_begin + blockIdx.x) * (BLOCK / 64) + (threadIdx.x >> 6)] =
            u32x4{n_live, n_bad, n_present - n_live, 0u};
}

// one workgroup per burst: the sum of the records its MAC workgroups left
__global__ __launch_bounds__(BLOCK) void cop_aead_status(const CopKAead p)
{
    __shared__ uint32_t red[BLOCK / 64][3];
    const CopKAeBurst &B = p.b[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t nrec = ((B.n_frames + BLOCK - 1) / BLOCK) * (BLOCK / 64);
    const u32x4 *const rec = (const u32x4 *)p.scratch + (size_t)(p.scratch_begin + B.mac_begin) * (BLOCK / 64);
    uint32_t done = 0, bad = 0, skipped = 0;
    for (uint32_t i = tid; i < nrec; i += BLOCK) {
        const u32x4 r = rec[i];
        done += r.x, bad += r.y, skipped += r.z;
    }
    done = wave_sum(done), bad = wave_sum(bad), skipped = wave_sum(skipped);
    if (lane == 0) red[wave][0] = done, red[wave][1] = bad, red[wave][2] = skipped;
    __syncthreads();
    if (tid == 0) {
        u32x4 s = u32x4{0u, 0u, 0u, 0u};
        for (int w = 0; w < BLOCK / 64; w++) s.x += red[w][0], s.y += red[w][1], s.z += red[w][2];
        *(u32x4 *)B.status = s;
    }
}

}  // namespace

extern "C" hipError_t copk_aead_launch(const CopKAead *pp, hipStream_t stream)
{
    const CopKAead &p = *pp;
    if (!p.nb) return hipSuccess;
    if (p.nb > COPK_AE_MAXB || p.mode > COPK_AE_POLY || !p.scratch) return hipErrorInvalidValue;
    for (uint32_t i = 0; i < p.nb; i++) {
        const uint32_t g = p.b[i].group;
        if (!p.b[i].n_frames || !g || g > 32u || (g & (g - 1u))) return hipErrorInvalidValue;
    }
    if (p.mode == COPK_AE_SEAL && p.xor_chunks) {
        hipLaunchKernelGGL(cop_aead_xor, dim3(p.xor_chunks), dim3(BLOCK), 0, stream, p);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    }
    if (p.mac_chunks) {
        hipLaunchKernelGGL(cop_aead_mac, dim3(p.mac_chunks), dim3(BLOCK), 0, stream, p);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    }
    if (p.mode == COPK_AE_OPEN && p.xor_chunks) {
        hipLaunchKernelGGL(cop_aead_xor, dim3(p.xor_chunks), dim3(BLOCK), 0, stream, p);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(cop_aead_status, dim3(p.nb), dim3(BLOCK), 0, stream, p);
    return hipGetLastError();
}
