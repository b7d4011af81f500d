// errorlocator_kernel.hip -- the genie-aided SC error locator on CDNA4 (gfx950), batched.
//
// The reference's PolarCode::Decoding::ErrorLocator (errorlocator.cpp) with lane = one codeword,
// as depthfirst_kernel: a wave decodes 64 frames at once and walks the SC-Flip plan's schedule
// (plan.cpp depthfirst_emit: the unpruned SC tree in decode order, F / G / combine of the nodes
// above size 8, one op per size-8 subtree) uniformly.  A leaf (Bit::decode, :153) outputs
// `replace ? desired : llr` as a whole word; a frozen leaf always replaces.
//
// One pass.  The reference's decode() repeats the root decode, each time marking the first
// unreplaced information leaf whose sign differs from its desired value's, until none is left
// (:219-222, findErrors :261-279).  SC is causal: replacing leaf i changes nothing before i, so
// the leaves are marked in ascending order and the last decode of that loop equals one decode in
// which every information leaf is compared when it is reached and replaced on the spot.  That is
// what EL_CORRECT does; the first leaf replaced and the number replaced are two registers of the
// lane.  A lane's replacements are data (a select at the leaf), never control flow.
//
// Per wave, a global slab of float4 units (words 4u .. 4u+3 of lane l at float4 [u * 64 + l]: a
// wave-wide unit access is one contiguous 1 KiB).  Per lane (errorlocator.hpp): the inputs of the
// nodes of each level (level 0 = the channel LLRs), the N decoded words, and the N desired
// values, each overwritten by its leaf's value once that leaf is done.  LLRs and desired values
// come in, and leaf values and decoded words go out, through one LDS transpose tile, so global
// accesses are contiguous runs of a frame's row (rows_in / rows_out of lane_frame.hpp, which also
// has the slab access and the launch; it comes through depthfirst_ops.hpp).
#include "errorlocator.hpp"

#include "depthfirst_ops.hpp"

namespace pcg {

namespace {

// what a lane carries through the leaves: firstError() and correctionCount()
struct Genie {
    int32_t first;
    uint32_t count;
};

// ShortRateRNode::decode (:135-143) over n values down to the single-bit leaves (Bit::decode :153).
// mask: the frozen leaves of the size-8 subtree, off: this node's first leaf in it, des / val: the
// desired and the output words of its eight leaves, idx0: the index of its first leaf among all N.
template <uint32_t n, uint32_t off>
PCG_DEV void el_small(const float* x, uint32_t* out, uint32_t mask, const uint32_t* des, uint32_t* val, uint32_t mode,
                      uint32_t idx0, Genie& g)
{
    if constexpr (n == 1) {
        const uint32_t d = des[off], v = fbits(x[0]);
        if ((mask >> off) & 1u) { // frozen: mReplace is always set
            out[0] = val[off] = d;
            return;
        }
        // findErrors / findFirstError: the sign bits differ (signEq :259)
        const bool miss = mode != EL_REFERENCE && ((d ^ v) >> 31) != 0;
        g.first = miss && g.first < 0 ? (int32_t)(idx0 + off) : g.first;
        g.count += miss && mode == EL_CORRECT ? 1u : 0u;
        out[0] = val[off] = miss && mode == EL_CORRECT ? d : v;
    } else {
        constexpr uint32_t h = n / 2;
        float y[h];
        uint32_t lb[h], rb[h];
#pragma unroll
        for (uint32_t i = 0; i < h; ++i)
            y[i] = polar_f(x[i], x[h + i]);
        el_small<h, off>(y, lb, mask, des, val, mode, idx0, g);
#pragma unroll
        for (uint32_t i = 0; i < h; ++i)
            y[i] = polar_g(x[i], x[h + i], lb[i] & 0x80000000u);
        el_small<h, off + h>(y, rb, mask, des, val, mode, idx0, g);
#pragma unroll
        for (uint32_t i = 0; i < h; ++i) {
            out[i] = lb[i] ^ rb[i];
            out[h + i] = rb[i];
        }
    }
}

PCG_DEV void el_leaf8_op(float* sf, uint32_t N, uint32_t l, uint32_t group, uint32_t mask, uint32_t mode,
                         bool has_desired, bool want_u, Genie& g)
{
    const uint32_t in = df_lvl(N, l), bp = df_bits(N) + group * 8u, dp = el_des(N) + group * 8u;
    const Vec<4> u = ldv<4>(sf, in), v = ldv<4>(sf, in + 4);
    float x[8];
    uint32_t des[8], val[8], out[8];
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
        x[k] = u.v[k];
        x[4 + k] = v.v[k];
    }
    if (has_desired) {
        const Vec<4> d0 = ldv<4>(sf, dp), d1 = ldv<4>(sf, dp + 4);
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
            des[k] = fbits(d0.v[k]);
            des[4 + k] = fbits(d1.v[k]);
        }
    } else { // pushBit (:239-246): +inf at a frozen leaf, +0 at an information leaf
#pragma unroll
        for (uint32_t k = 0; k < 8; ++k)
            des[k] = (mask >> k) & 1u ? 0x7f800000u : 0u;
    }
    el_small<8, 0>(x, out, mask, des, val, mode, group * 8u, g);
    Vec<4> r0, r1;
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
        r0.v[k] = ubits(out[k]);
        r1.v[k] = ubits(out[4 + k]);
    }
    stv<4>(sf, bp, r0);
    stv<4>(sf, bp + 4, r1);
    if (want_u) {
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
            r0.v[k] = ubits(val[k]);
            r1.v[k] = ubits(val[4 + k]);
        }
        stv<4>(sf, dp, r0);
        stv<4>(sf, dp + 4, r1);
    }
}

__global__ void __launch_bounds__(64) errorlocator_kernel(ErrorLocatorArgs a)
{
    extern __shared__ uint32_t smem_el[];
    uint32_t* tile = smem_el;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t N = a.c.N, mode = a.mode;
    const uint32_t T = N < TILE ? N : TILE;
    float* sf = a.c.slab + (uint64_t)blockIdx.x * a.c.slab_floats * 64u + lane * 4u;
    const bool has_desired = a.desired != nullptr, want_u = a.u != nullptr;
    const uint64_t ngroups = (a.c.F + 63) / 64;
    for (uint64_t grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {
        const uint64_t frame0 = grp * 64, frame = frame0 + lane;
        const uint32_t nfr = a.c.F - frame0 < 64 ? (uint32_t)(a.c.F - frame0) : 64u;
        rows_in(tile, sf, 0, a.c.llr, frame0, nfr, N, T, lane);
        if (has_desired)
            rows_in(tile, sf, el_des(N), a.desired, frame0, nfr, N, T, lane);
        Genie g;
        g.first = -1;
        g.count = 0;
        for (uint32_t k = 0; k < a.c.nops; ++k) {
            const uint32_t op = ld_const(a.c.ops, DF_WORDS * k);
            const uint32_t code = scan_code(op), l = scan_level(op), grpn = scan_group(op);
            if (code == DF_F)
                rater_op<DF_F>(sf, N, l, grpn);
            else if (code == DF_G)
                rater_op<DF_G>(sf, N, l, grpn);
            else if (code == DF_COMB)
                rater_op<DF_COMB>(sf, N, l, grpn);
            else
                el_leaf8_op(sf, N, l, grpn, scan_flags(op), mode, has_desired, want_u, g);
        }
        if (lane < nfr) {
            if (a.first)
                a.first[frame] = g.first;
            if (a.count)
                a.count[frame] = g.count;
        }
        if (want_u)
            rows_out(tile, sf, el_des(N), reinterpret_cast<uint32_t*>(a.u), frame0, nfr, N, T, lane, ~0ull);
        if (a.bits)
            rows_out(tile, sf, df_bits(N), a.bits, frame0, nfr, N, T, lane, ~0ull);
    }
}

} // namespace

uint64_t errorlocator_wave_cap(uint32_t N, uint32_t slab_floats)
{
    return lane_wave_cap(errorlocator_kernel, lane_lds_bytes(N, false), 256ull * slab_floats);
}

int launch_errorlocator(const ErrorLocatorArgs& a, hipStream_t stream)
{
    return lane_launch(errorlocator_kernel, a, lane_lds_bytes(a.c.N, false), stream);
}

} // namespace pcg
