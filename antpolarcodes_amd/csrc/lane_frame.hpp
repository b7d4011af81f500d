// lane_frame.hpp -- what the lane = codeword kernels share (scan_kernel.hip, fsscan_kernel.hip,
// depthfirst_kernel.hip, errorlocator_kernel.hip): a wave of 64 lanes decodes 64 frames, each
// lane's state in a global slab of interleaved units.  Here: the transpose tile between F x N
// rows in global memory and the lanes' slabs, access to a slab of float4 units, the detector
// syndrome and the information bytes from a lane's sign-bit row, and the wave cap and the launch
// of such a kernel.  Nothing here knows which kernel calls it.
//
// Not part of the sources embedded for run-time compilation: wave.hpp, kernels.hpp and plan.hpp
// never include it.
#pragma once
#include "scan.hpp"
#include "wave.hpp"

namespace pcg {

constexpr uint32_t TILE = 64;        // positions per transpose tile
constexpr uint32_t TILE_STRIDE = 65; // LDS row stride of a tile (conflict-free columns)

// LDS bytes of a wave: the tile and, with_sign_rows, one row of N sign bits per lane
constexpr inline uint32_t lane_lds_bytes(uint32_t N, bool with_sign_rows)
{
    return 4u * (TILE * TILE_STRIDE + (with_sign_rows ? 64u * (N >= 32 ? N / 32 : 1u) : 0u));
}

namespace {

// ---- a lane's slab of float4 units: sf = slab + lane * 4, words 4u .. 4u+3 at float4 [u * 64] ----
// W consecutive words of a lane at slab offset `off` (a multiple of W; W = 4 or 2)
template <uint32_t W>
struct Vec {
    float v[W];
};
template <uint32_t W>
PCG_DEV Vec<W> ldv(const float* sf, uint32_t off)
{
    Vec<W> r;
    if constexpr (W == 4) {
        const float4 t = *reinterpret_cast<const float4*>(sf + (uint64_t)off * 64u);
        r.v[0] = t.x, r.v[1] = t.y, r.v[2] = t.z, r.v[3] = t.w;
    } else {
        const float2 t = *reinterpret_cast<const float2*>(sf + (uint64_t)(off >> 2) * 256u + (off & 3u));
        r.v[0] = t.x, r.v[1] = t.y;
    }
    return r;
}
template <uint32_t W>
PCG_DEV void stv(float* sf, uint32_t off, const Vec<W>& r)
{
    if constexpr (W == 4)
        *reinterpret_cast<float4*>(sf + (uint64_t)off * 64u) = make_float4(r.v[0], r.v[1], r.v[2], r.v[3]);
    else
        *reinterpret_cast<float2*>(sf + (uint64_t)(off >> 2) * 256u + (off & 3u)) = make_float2(r.v[0], r.v[1]);
}
// word i of the lane's slab (any i)
PCG_DEV float* wordp(float* sf, uint32_t i) { return sf + (uint64_t)(i >> 2) * 256u + (i & 3u); }

// ---- the transpose tile: tile[f * TILE_STRIDE + j] = position c * T + j of frame frame0 + f ----
// (T = min(N, TILE) positions per pass c; the values travel as 32-bit words)

// positions [c * T, c * T + T) of rows [frame0, frame0 + nfr) of the F x N array `src` into the
// tile; rows past nfr read as 0
PCG_DEV void tile_in(uint32_t* tile, const float* src, uint64_t frame0, uint32_t nfr, uint32_t N, uint32_t c,
                     uint32_t T, uint32_t lane)
{
    // a wave has no other wave on its SIMD to hide a load behind: 16 rows in flight at a time
    for (uint32_t f0 = 0; f0 < 64; f0 += 16) {
        uint32_t v[16];
#pragma unroll
        for (uint32_t q = 0; q < 16; ++q)
            v[q] = lane < T && f0 + q < nfr ? fbits(src[(frame0 + f0 + q) * N + c * T + lane]) : 0u;
#pragma unroll
        for (uint32_t q = 0; q < 16; ++q)
            if (lane < T)
                tile[(f0 + q) * TILE_STRIDE + lane] = v[q];
    }
    wsync();
}

// the tile (row `lane` written by lane `lane`) to the same positions of the rows of `dst` whose
// frame has its bit set in `mask`
PCG_DEV void tile_out(const uint32_t* tile, uint32_t* dst, uint64_t frame0, uint32_t nfr, uint32_t N, uint32_t c,
                      uint32_t T, uint32_t lane, uint64_t mask)
{
    wsync();
    for (uint32_t f = 0; f < nfr; ++f)
        if (((mask >> f) & 1u) && lane < T)
            dst[(frame0 + f) * N + c * T + lane] = tile[f * TILE_STRIDE + lane];
    wsync();
}

// rows [frame0, frame0 + nfr) of the F x N array `src` into words [base, base + N) of the lanes' slabs
PCG_DEV void rows_in(uint32_t* tile, float* sf, uint32_t base, const float* src, uint64_t frame0, uint32_t nfr,
                     uint32_t N, uint32_t T, uint32_t lane)
{
    for (uint32_t c = 0; c < N / T; ++c) {
        tile_in(tile, src, frame0, nfr, N, c, T, lane);
        for (uint32_t j = 0; j < T; j += 4) {
            Vec<4> v;
#pragma unroll
            for (uint32_t k = 0; k < 4; ++k)
                v.v[k] = ubits(tile[lane * TILE_STRIDE + j + k]);
            stv<4>(sf, base + c * T + j, v);
        }
        wsync();
    }
}

// the same where the rows are 16-byte aligned (src is, and N is a multiple of 8, so the tail is two
// float4): every lane reads its own row, eight float4 in flight (the loads of a wave are what a
// one-wave-per-CU launch waits for: 32 round trips at N = 1024 instead of the tile's 1024 row loads)
PCG_DEV void rows_in_own(float* sf, uint32_t base, const float* src, uint64_t frame0, uint32_t nfr, uint32_t N,
                         uint32_t lane)
{
    const float4* row = reinterpret_cast<const float4*>(src + (frame0 + (lane < nfr ? lane : 0u)) * N);
    for (uint32_t e = 0; e < N; e += 32) {
        float4 v[8];
#pragma unroll
        for (uint32_t q = 0; q < 8; ++q)
            if (e + 4 * q < N)
                v[q] = row[(e >> 2) + q];
#pragma unroll
        for (uint32_t q = 0; q < 8; ++q)
            if (e + 4 * q < N)
                *reinterpret_cast<float4*>(sf + (uint64_t)(base + e + 4 * q) * 64u) =
                    lane < nfr ? v[q] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
}

// words [base, base + N) of the lanes' slabs into the rows of the F x N array `dst` whose frame has
// its bit set in `mask`
PCG_DEV void rows_out(uint32_t* tile, const float* sf, uint32_t base, uint32_t* dst, uint64_t frame0, uint32_t nfr,
                      uint32_t N, uint32_t T, uint32_t lane, uint64_t mask)
{
    for (uint32_t c = 0; c < N / T; ++c) {
        for (uint32_t j = 0; j < T; j += 4) {
            const Vec<4> x = ldv<4>(sf, base + c * T + j);
#pragma unroll
            for (uint32_t k = 0; k < 4; ++k)
                tile[lane * TILE_STRIDE + j + k] = fbits(x.v[k]);
        }
        tile_out(tile, dst, frame0, nfr, N, c, T, lane, mask);
    }
}

// ---- a lane's sign-bit row in LDS: word q (positions 32q .. 32q + 31, LSB first) at row[q * 64] ----

// the detector syndrome of the row's W words: crc_c0 ^ parity(row & crc_rows[rb]) per detector bit
PCG_DEV uint32_t detector_syndrome(const uint32_t* row, uint32_t W, uint32_t crc_c0, uint32_t crc_bits,
                                   const uint32_t* crc_rows)
{
    uint32_t syn = crc_c0;
    for (uint32_t rb = 0; rb < crc_bits; ++rb) {
        uint32_t pc = 0;
        for (uint32_t q = 0; q < W; ++q)
            pc += __builtin_popcount(row[q << 6] & crc_rows[rb * W + q]);
        syn ^= (pc & 1u) << rb;
    }
    return syn;
}

// the K information bits (positions info_pos, ascending) of the row, MSB first, into out[0, kb)
PCG_DEV void store_info_bytes(const uint32_t* row, const uint16_t* info_pos, uint32_t K, uint32_t kb, uint8_t* out)
{
    uint32_t cw = 0xffffffffu, word = 0;
    for (uint32_t b = 0; b < kb; ++b) {
        uint32_t byte = 0;
        for (uint32_t q = 0; q < 8; ++q) {
            const uint32_t idx = 8 * b + q;
            if (idx < K) {
                const uint32_t pos = info_pos[idx];
                if ((pos >> 5) != cw) {
                    cw = pos >> 5;
                    word = row[cw << 6];
                }
                byte |= ((word >> (pos & 31u)) & 1u) << (7 - q);
            }
        }
        out[b] = (uint8_t)byte;
    }
}

// ---- host side ----

// Persistent waves of a launch: up to 4 per CU (one per SIMD) as far as they are resident, and
// as many as keep the slabs (slab_bytes per wave) within 2 GiB.
template <typename Kernel>
uint64_t lane_wave_cap(Kernel kernel, uint32_t lds_bytes, uint64_t slab_bytes)
{
    int dev = 0, cus = 256, res = 0;
    if (hipGetDevice(&dev) == hipSuccess)
        (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&res, kernel, 64, lds_bytes) != hipSuccess)
        res = 0;
    uint64_t wpc = res > 0 ? (uint64_t)res : 1;
    if (wpc > 4)
        wpc = 4;
    uint64_t cap = (uint64_t)cus * wpc;
    const uint64_t fit = (2ull << 30) / slab_bytes;
    if (cap > fit)
        cap = fit ? fit : 1;
    return cap;
}

// one wave per grid unit; -4 no unit for F frames, -3 the launch failed
template <typename Args>
int lane_launch(void (*kernel)(Args), const Args& a, uint32_t lds_bytes, hipStream_t stream)
{
    if (a.c.units == 0)
        return a.c.F ? -4 : 0;
    hipLaunchKernelGGL(kernel, dim3(a.c.units), dim3(64), (size_t)lds_bytes, stream, a);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

} // namespace

} // namespace pcg
