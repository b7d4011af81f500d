// depthfirst_ops.hpp -- device code shared by the kernels that walk plan.cpp's depthfirst_emit
// schedule with lane = codeword (depthfirst_kernel.hip, errorlocator_kernel.hip): the F / G /
// combine ops of the nodes above size 8.  The access to a lane's slab of float4 units and the frame
// I/O come with lane_frame.hpp.
#pragma once
#include "depthfirst.hpp"
#include "lane_frame.hpp"

namespace pcg {

namespace {

// F / G / combine of a node over the values [i0, i0 + 4B) of its halves: inputs (a | b) at `in`,
// the child's input at `nx`, the node's words at `bp`
template <uint32_t CODE, uint32_t B>
PCG_DEV void rater_chunk(float* sf, uint32_t in, uint32_t h, uint32_t nx, uint32_t bp, uint32_t i0)
{
    Vec<4> a[B], b[B], s[B];
#pragma unroll
    for (uint32_t q = 0; q < B; ++q) {
        const uint32_t i = i0 + 4 * q;
        if (CODE != DF_COMB) {
            a[q] = ldv<4>(sf, in + i);
            b[q] = ldv<4>(sf, in + h + i);
        }
        if (CODE == DF_G)
            s[q] = ldv<4>(sf, bp + i);
        if (CODE == DF_COMB) {
            a[q] = ldv<4>(sf, bp + i);
            b[q] = ldv<4>(sf, bp + h + i);
        }
    }
#pragma unroll
    for (uint32_t q = 0; q < B; ++q) {
        const uint32_t i = i0 + 4 * q;
        Vec<4> r;
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
            if (CODE == DF_F)
                r.v[k] = polar_f(a[q].v[k], b[q].v[k]);
            else if (CODE == DF_G)
                r.v[k] = polar_g(a[q].v[k], b[q].v[k], sgn(s[q].v[k]));
            else
                r.v[k] = ubits(fbits(a[q].v[k]) ^ fbits(b[q].v[k]));
        }
        stv<4>(sf, CODE == DF_COMB ? bp + i : nx + i, r);
    }
}

template <uint32_t CODE>
PCG_DEV void rater_op(float* sf, uint32_t N, uint32_t l, uint32_t group)
{
    const uint32_t n = N >> l, h = n >> 1; // h >= 8
    const uint32_t in = df_lvl(N, l), nx = df_lvl(N, l + 1), bp = df_bits(N) + group * n;
    uint32_t i = 0;
    for (; i + 16 <= h; i += 16)
        rater_chunk<CODE, 4>(sf, in, h, nx, bp, i);
    for (; i < h; i += 4)
        rater_chunk<CODE, 1>(sf, in, h, nx, bp, i);
}

} // namespace

} // namespace pcg
