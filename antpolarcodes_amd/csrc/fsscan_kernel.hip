// fsscan_kernel.hip -- batched Fast-SSCAN soft-output polar decoding on CDNA4 (gfx950).
//
// The reference's PolarCode::Decoding::FastSscanFloat (fastsscan_float.cpp) with lane = one
// codeword, as scan_kernel: a wave decodes 64 frames at once and walks the plan's schedule
// (plan.cpp fsscan_emit: RateRNode::decode written out in decode order, one op per phase, plus
// one op per Repetition and TwoBit node) uniformly, every lane running the reference's fp32
// expressions on its own state.  Zero and One nodes are never visited: their messages (+inf, +0)
// are constant operands of their parents' expressions, which are computed, not special-cased.
//
// Per wave, a global slab of float4 units (floats 4u .. 4u+3 of lane l at float4 [u * 64 + l]: a
// wave-wide unit access is one contiguous 1 KiB).  Per lane (fsscan.hpp): IN, the inputs of the
// nodes of each level (level 0 = the channel LLRs, kept for the output); EL, the messages of the
// root and of the left children per level; then the messages of the right children, the only
// state that lives across passes.  Nothing is zeroed: every IN and EL value is written before
// it is read in every pass, and the first pass takes a right child's message as the +0 that
// reset() leaves where its left sibling's input is computed (also for a TwoBit node, whose
// reset() is empty in the reference: DESIGN.md Q list).
//
// A pass is repeated while the frame's detector check fails, up to the trial limit; a wave runs
// until all of its lanes have passed.  A lane that has passed keeps computing with the wave, but
// its outputs are stored only in passes it still needed.
//
// The tile's store to frame rows, the slab access (Vec / ldv / stv), the detector syndrome, the
// information bytes and the launch are lane_frame.hpp's; the fused "soft = llr + root message,
// sign bits" loop in front of the soft codeword's store and the channel load stay here.
#include "fsscan.hpp"
#include "lane_frame.hpp"

namespace pcg {

namespace {

template <uint32_t W>
PCG_DEV Vec<W> splat(float c)
{
    Vec<W> r;
#pragma unroll
    for (uint32_t q = 0; q < W; ++q)
        r.v[q] = c;
    return r;
}

// the three phases of a RateR node over the values [i0, i0 + B * W) of its halves: in = (a | b)
// at `in`, the children's messages at el / er (or the constants elc / erc)
template <uint32_t CODE, uint32_t W, uint32_t B>
PCG_DEV void rater_chunk(float* sf, uint32_t in, uint32_t h, uint32_t el, uint32_t er, uint32_t dst, uint32_t i0,
                         bool el_ld, float elc, bool er_ld, float erc)
{
    Vec<W> a[B], b[B], e[B], o[B];
#pragma unroll
    for (uint32_t q = 0; q < B; ++q) {
        const uint32_t i = i0 + q * W;
        a[q] = ldv<W>(sf, in + i);
        b[q] = ldv<W>(sf, in + h + i);
        if (CODE != FSS_LEFT)
            e[q] = el_ld ? ldv<W>(sf, el + i) : splat<W>(elc);
        if (CODE != FSS_RIGHT)
            o[q] = er_ld ? ldv<W>(sf, er + i) : splat<W>(erc);
    }
#pragma unroll
    for (uint32_t q = 0; q < B; ++q) {
        const uint32_t i = i0 + q * W;
        Vec<W> r, s;
#pragma unroll
        for (uint32_t k = 0; k < W; ++k) {
            if (CODE == FSS_LEFT) {
                r.v[k] = polar_f(o[q].v[k] + b[q].v[k], a[q].v[k]);
            } else if (CODE == FSS_RIGHT) {
                r.v[k] = polar_f(e[q].v[k], a[q].v[k]) + b[q].v[k];
            } else {
                r.v[k] = polar_f(e[q].v[k], o[q].v[k] + b[q].v[k]);
                s.v[k] = o[q].v[k] + polar_f(e[q].v[k], a[q].v[k]);
            }
        }
        stv<W>(sf, dst + i, r);
        if (CODE == FSS_OUT)
            stv<W>(sf, dst + h + i, s);
    }
}

template <uint32_t CODE>
PCG_DEV void rater_op(float* sf, uint32_t N, uint32_t l, uint32_t fl, uint32_t er, uint32_t own, bool first)
{
    const float inf = __builtin_inff();
    const uint32_t h = N >> (l + 1);
    const uint32_t in = fsscan_lvl(N, l);
    const uint32_t el = fsscan_el(N) + fsscan_lvl(N, l + 1);
    const uint32_t dst = CODE == FSS_OUT ? own : fsscan_lvl(N, l + 1);
    const bool el_ld = !(fl & (FSS_L_ZERO | FSS_L_ONE));
    const float elc = (fl & FSS_L_ZERO) ? inf : 0.0f;
    // the right child's message: what the previous pass left (reset()'s +0 in the first pass)
    // where the left child's input is computed, this pass's afterwards
    const bool er_ld = !(fl & (FSS_R_ZERO | FSS_R_ONE)) && !(CODE == FSS_LEFT && first);
    const float erc = (fl & FSS_R_ZERO) ? inf : 0.0f;
    if (h == 2) {
        rater_chunk<CODE, 2, 1>(sf, in, h, el, er, dst, 0, el_ld, elc, er_ld, erc);
        return;
    }
    uint32_t i = 0;
    for (; i + 16 <= h; i += 16)
        rater_chunk<CODE, 4, 4>(sf, in, h, el, er, dst, i, el_ld, elc, er_ld, erc);
    for (; i < h; i += 4)
        rater_chunk<CODE, 4, 1>(sf, in, h, el, er, dst, i, el_ld, elc, er_ld, erc);
}

// RepetitionNode::decode: the sum in the reference's order (left to right below 8 values, else
// eight interleaved partial sums added left to right), then sum - in
PCG_DEV void rep_op(float* sf, uint32_t in, uint32_t n, uint32_t dst)
{
    float s;
    if (n < 8) {
        const Vec<4> v = ldv<4>(sf, in);
        s = 0.0f;
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k)
            s += v.v[k];
    } else {
        float p[8];
#pragma unroll
        for (uint32_t k = 0; k < 8; ++k)
            p[k] = 0.0f;
        for (uint32_t i = 0; i < n; i += 8) {
            const Vec<4> u = ldv<4>(sf, in + i), v = ldv<4>(sf, in + i + 4);
#pragma unroll
            for (uint32_t k = 0; k < 4; ++k) {
                p[k] += u.v[k];
                p[4 + k] += v.v[k];
            }
        }
        s = p[0] + p[1];
#pragma unroll
        for (uint32_t k = 2; k < 8; ++k)
            s += p[k];
    }
    for (uint32_t i = 0; i < n; i += 4) {
        Vec<4> v = ldv<4>(sf, in + i);
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k)
            v.v[k] = s - v.v[k];
        stv<4>(sf, dst + i, v);
    }
}

__global__ void __launch_bounds__(64) fsscan_kernel(FsscanArgs a)
{
    extern __shared__ uint32_t smem_fsscan[];
    uint32_t* tile = smem_fsscan;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t N = a.c.N;
    const uint32_t T = N < TILE ? N : TILE;
    const uint32_t W = N >= 32 ? N / 32 : 1u;
    uint32_t* row = smem_fsscan + TILE * TILE_STRIDE + lane; // own sign-bit row, word q at [q * 64]
    float* sf = a.c.slab + (uint64_t)blockIdx.x * a.c.slab_floats * 64u + lane * 4u;
    const uint32_t IN0 = 0, OUT0 = fsscan_el(N); // channel LLRs, the root's message
    const uint64_t ngroups = (a.c.F + 63) / 64;
    const bool aligned = (reinterpret_cast<uintptr_t>(a.c.llr) & 15u) == 0; // rows are N * 4 bytes, N >= 8
    for (uint64_t grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {
        const uint64_t frame0 = grp * 64, frame = frame0 + lane;
        const uint32_t nfr = a.c.F - frame0 < 64 ? (uint32_t)(a.c.F - frame0) : 64u;
        // channel LLRs into level 0.  Rows that are 16-byte aligned: every lane reads its own frame,
        // eight float4 in flight (the loads of a wave are what a one-wave-per-CU launch waits for:
        // 32 round trips at N = 1024 instead of the tile's 1024 row loads); else through the tile, one
        // row load at a time.  Both stay here (not lane_frame.hpp's rows_in_own / rows_in): with
        // rows_in the scalar registers of its 16 loads in flight were spilled inside the passes'
        // loops, +3 % per pass, and with rows_in_own a one-pass decode still measured 0.2 - 0.4 %
        // over its bound (profiles/lane_frame_refactor.txt)
        if (aligned) {
            const float4* src = reinterpret_cast<const float4*>(a.c.llr + (lane < nfr ? frame : frame0) * N);
            for (uint32_t e = 0; e < N; e += 32) { // N is a multiple of 8: the tail is two float4
                float4 v[8];
#pragma unroll
                for (uint32_t q = 0; q < 8; ++q)
                    if (e + 4 * q < N)
                        v[q] = src[(e >> 2) + q];
#pragma unroll
                for (uint32_t q = 0; q < 8; ++q)
                    if (e + 4 * q < N)
                        *reinterpret_cast<float4*>(sf + (uint64_t)(IN0 + e + 4 * q) * 64u) =
                            lane < nfr ? v[q] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            }
        }
        for (uint32_t c = 0; !aligned && c < N / T; ++c) {
            for (uint32_t f = 0; f < 64; ++f)
                if (lane < T)
                    tile[f * TILE_STRIDE + lane] = f < nfr ? fbits(a.c.llr[(frame0 + f) * N + c * T + lane]) : 0u;
            wsync();
            for (uint32_t j = 0; j < T; j += 4) {
                Vec<4> v;
#pragma unroll
                for (uint32_t k = 0; k < 4; ++k)
                    v.v[k] = ubits(tile[lane * TILE_STRIDE + j + k]);
                stv<4>(sf, IN0 + c * T + j, v);
            }
            wsync();
        }
        bool done = lane >= nfr; // passed its check in an earlier pass (or no frame)
        for (uint32_t pass = 1; pass <= a.trials; ++pass) {
            const bool first = pass == 1;
            for (uint32_t k = 0; k < a.c.nops; ++k) {
                const uint32_t op = ld_const(a.c.ops, FSS_WORDS * k), er = ld_const(a.c.ops, FSS_WORDS * k + 1),
                               own = ld_const(a.c.ops, FSS_WORDS * k + 2);
                const uint32_t code = scan_code(op), l = scan_level(op), fl = scan_flags(op);
                if (code == FSS_LEFT) {
                    rater_op<FSS_LEFT>(sf, N, l, fl, er, own, first);
                } else if (code == FSS_RIGHT) {
                    rater_op<FSS_RIGHT>(sf, N, l, fl, er, own, first);
                } else if (code == FSS_OUT) {
                    rater_op<FSS_OUT>(sf, N, l, fl, er, own, first);
                } else if (code == FSS_REP) {
                    rep_op(sf, IN0 + fsscan_lvl(N, l), N >> l, own);
                } else if (code == FSS_TWO) {
                    const Vec<2> v = ldv<2>(sf, IN0 + fsscan_lvl(N, l));
                    Vec<2> r;
                    r.v[0] = v.v[1], r.v[1] = v.v[0];
                    stv<2>(sf, own, r);
                } else { // FSS_CONST: the root is a Zero or a One node
                    const Vec<4> v = splat<4>((fl & FSS_L_ZERO) ? __builtin_inff() : 0.0f);
                    for (uint32_t i = 0; i < N; i += 4)
                        stv<4>(sf, own + i, v);
                }
            }
            const bool last = pass == a.trials;
            if (a.forced && !last)
                continue;
            // calculateOutput: soft = llr + root message and its sign bits; lanes still
            // decoding store theirs (a later pass of the same lane overwrites it)
            const bool live = !done;
            const uint64_t livem = ballot(live);
            for (uint32_t c = 0; c < N / T; ++c) {
                uint32_t bits = 0;
                for (uint32_t j = 0; j < T; j += 4) {
                    const Vec<4> x = ldv<4>(sf, IN0 + c * T + j), m = ldv<4>(sf, OUT0 + c * T + j);
#pragma unroll
                    for (uint32_t k = 0; k < 4; ++k) {
                        const float v = x.v[k] + m.v[k];
                        bits |= (fbits(v) >> 31) << ((j + k) & 31u);
                        if (a.soft)
                            tile[lane * TILE_STRIDE + j + k] = fbits(v);
                    }
                    if (((j + 3) & 31u) == 31u || j + 4 == T) {
                        row[((c * T + j) >> 5) << 6] = bits;
                        bits = 0;
                    }
                }
                if (a.soft)
                    tile_out(tile, reinterpret_cast<uint32_t*>(a.soft), frame0, nfr, N, c, T, lane, livem);
            }
            // detector syndrome and info bytes from the sign bits
            const bool pass_ok = detector_syndrome(row, W, a.c.crc_c0, a.c.crc_bits, a.c.crc_rows) == 0;
            if (live && (a.forced || pass_ok || last)) { // this lane's final pass
                store_info_bytes(row, a.c.info_pos, a.c.K, a.c.kb, a.c.info + frame * a.c.kb);
                if (a.c.ok)
                    a.c.ok[frame] = pass_ok ? 1 : 0;
                if (a.ntrials)
                    a.ntrials[frame] = (uint8_t)pass;
            }
            if (!a.forced) {
                done = done || pass_ok;
                if (ballot(!done) == 0)
                    break;
            }
        }
    }
}

} // namespace

uint64_t fsscan_wave_cap(uint32_t N, uint32_t slab_floats)
{
    return lane_wave_cap(fsscan_kernel, lane_lds_bytes(N, true), 256ull * slab_floats);
}

int launch_fsscan(const FsscanArgs& a, hipStream_t stream)
{
    return lane_launch(fsscan_kernel, a, lane_lds_bytes(a.c.N, true), stream);
}

} // namespace pcg
