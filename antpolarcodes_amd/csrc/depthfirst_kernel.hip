// depthfirst_kernel.hip -- batched SC-Flip polar decoding on CDNA4 (gfx950).
//
// The reference's PolarCode::Decoding::DepthFirst (depth_first.cpp) with lane = one codeword, as
// fsscan_kernel: a wave decodes 64 frames at once and walks the plan's schedule (plan.cpp
// depthfirst_emit: the unpruned SC tree in decode order, F / G / combine of the nodes above size
// 8, one op per size-8 subtree) uniformly, every lane running the reference's fp32 expressions
// on its own state.  The decoded "bits" are 32-bit words: an information leaf outputs its LLR
// (negated when its option is 1), a frozen leaf +inf, a node the XOR of its children's words.
//
// Per wave, a global slab of float4 units (words 4u .. 4u+3 of lane l at float4 [u * 64 + l]: a
// wave-wide unit access is one contiguous 1 KiB).  Per lane (depthfirst.hpp): the inputs of the
// nodes of each level (level 0 = the channel LLRs), the N decoded words, the K reliabilities of
// the first pass, and the search entries.  Every trial is a full root decode.
//
// The search (Manager::decode / decodeNext) per lane, in the reduced form that
// tests/depthfirst_numpy.py shows equal to the reference's queue: entry k is the configuration
// trial k + 1 decodes -- its prefix leaves, options and depth.  The first pass's order gives the
// depth-0 entries; each later pop of a depth-0 entry adds two children with the least reliable
// leaf outside its prefix, found while that entry is decoded; children of deeper entries only
// count.  A lane's flips are data (a select at the information leaves), never control flow.
// Ties go to the lower leaf index.
//
// A wave runs until all of its lanes have passed their check or used their trials.  A lane that
// has passed keeps computing with the wave; its outputs are stored once, in its last trial.
//
// Frame rows in and out through the transpose tile, the slab access, the detector syndrome, the
// information bytes and the launch are lane_frame.hpp's (through depthfirst_ops.hpp).
#include "depthfirst_ops.hpp"

namespace pcg {

namespace {

constexpr uint32_t NO_LEAF = 0xffffu;

// what a lane carries through the leaves of one root decode
struct LeafState {
    uint32_t f0, f1; // information ranks whose option is 1 (NO_LEAF: none)
    uint32_t excl;   // the rank left out of the min-selection (NO_LEAF: none)
    float best;      // the least reliability outside excl so far, and its rank (strict <: ties to
    uint32_t besti;  // the lower rank)
};

// ShortRateRNode::decode over n values down to the single-bit leaves (RateZeroDecoder: +inf;
// RateOneDecoder of block length 1: the LLR, negated when its option is 1; reliability |LLR|).
// mask: the frozen leaves of the size-8 subtree, off: this node's first leaf in it.
template <uint32_t n, uint32_t off>
PCG_DEV void sc_small(const float* x, uint32_t* out, uint32_t mask, uint32_t rank0, LeafState& c, float* rel)
{
    if constexpr (n == 1) {
        if ((mask >> off) & 1u) {
            out[0] = 0x7f800000u;
            return;
        }
        const uint32_t r = rank0 + __builtin_popcount(~mask & ((1u << off) - 1u));
        const float m = fabs_(x[0]);
        if (rel)
            *wordp(rel, r) = m;
        if (r != c.excl && m < c.best) {
            c.best = m;
            c.besti = r;
        }
        out[0] = fbits(x[0]) ^ ((r == c.f0 || r == c.f1) ? 0x80000000u : 0u);
    } else {
        constexpr uint32_t h = n / 2;
        float y[h];
        uint32_t lb[h], rb[h];
#pragma unroll
        for (uint32_t i = 0; i < h; ++i)
            y[i] = polar_f(x[i], x[h + i]);
        sc_small<h, off>(y, lb, mask, rank0, c, rel);
#pragma unroll
        for (uint32_t i = 0; i < h; ++i)
            y[i] = polar_g(x[i], x[h + i], lb[i] & 0x80000000u);
        sc_small<h, off + h>(y, rb, mask, rank0, c, rel);
#pragma unroll
        for (uint32_t i = 0; i < h; ++i) {
            out[i] = lb[i] ^ rb[i];
            out[h + i] = rb[i];
        }
    }
}

PCG_DEV void leaf8_op(float* sf, uint32_t N, uint32_t l, uint32_t group, uint32_t mask, uint32_t rank0, LeafState& c,
                      float* rel)
{
    const uint32_t in = df_lvl(N, l), bp = df_bits(N) + group * 8u;
    const Vec<4> u = ldv<4>(sf, in), v = ldv<4>(sf, in + 4);
    float x[8];
    uint32_t out[8];
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
        x[k] = u.v[k];
        x[4 + k] = v.v[k];
    }
    sc_small<8, 0>(x, out, mask, rank0, c, rel);
    Vec<4> r0, r1;
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
        r0.v[k] = ubits(out[k]);
        r1.v[k] = ubits(out[4 + k]);
    }
    stv<4>(sf, bp, r0);
    stv<4>(sf, bp + 4, r1);
}

// the leaf after `pv, pi` in (reliability, rank) order among the K first-pass reliabilities
PCG_DEV void next_weakest(const float* rel, uint32_t K, float pv, uint32_t pi, float& v, uint32_t& i)
{
    float bv = __builtin_inff();
    uint32_t bi = NO_LEAF;
    for (uint32_t r = 0; r < K; r += 4) {
        const Vec<4> q = ldv<4>(rel, r);
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
            const float m = q.v[k];
            const bool after = m > pv || (m == pv && r + k > pi);
            if (r + k < K && after && (bi == NO_LEAF || m < bv)) {
                bv = m;
                bi = r + k;
            }
        }
    }
    v = bv;
    i = bi;
}

PCG_DEV uint32_t entry0(uint32_t n0, uint32_t opt) { return n0 | (0xfffu << 12) | (opt ? DF_E_OPT0 : 0u); }

__global__ void __launch_bounds__(64) depthfirst_kernel(DepthFirstArgs a)
{
    extern __shared__ uint32_t smem_df[];
    uint32_t* tile = smem_df;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t N = a.c.N, K = a.c.K, TL = a.trials;
    const uint32_t T = N < TILE ? N : TILE;
    const uint32_t W = N >= 32 ? N / 32 : 1u;
    uint32_t* row = smem_df + TILE * TILE_STRIDE + lane; // own sign-bit row, word q at [q * 64]
    float* sf = a.c.slab + (uint64_t)blockIdx.x * a.c.slab_floats * 64u + lane * 4u;
    float* rel = sf + (uint64_t)df_rel(N) * 64u;
    float* ent = sf + (uint64_t)df_ent(N, K) * 64u;
    const uint32_t BITS = df_bits(N);
    const double log9 = 2.1972245773362196; // log(9): the reference compares in double
    const uint64_t ngroups = (a.c.F + 63) / 64;
    const bool aligned = (reinterpret_cast<uintptr_t>(a.c.llr) & 15u) == 0; // rows are N * 4 bytes, N >= 8
    for (uint64_t grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {
        const uint64_t frame0 = grp * 64, frame = frame0 + lane;
        const uint32_t nfr = a.c.F - frame0 < 64 ? (uint32_t)(a.c.F - frame0) : 64u;
        // channel LLRs into level 0: own rows when 16-byte aligned, else through the tile
        if (aligned)
            rows_in_own(sf, 0, a.c.llr, frame0, nfr, N, lane);
        else
            rows_in(tile, sf, 0, a.c.llr, frame0, nfr, N, T, lane);
        bool done = lane >= nfr; // passed its check in an earlier trial (or no frame)
        LeafState ls;
        ls.f0 = ls.f1 = ls.excl = NO_LEAF;
        uint32_t ord1 = 0;             // the second weakest leaf of the first pass
        uint32_t qsize = 0, ecount = 0; // the reference's queue size; entries pushed so far
        for (uint32_t run = 1; run <= TL; ++run) {
            ls.best = __builtin_inff();
            ls.besti = NO_LEAF;
            float* relw = run == 1 && TL > 1 ? rel : nullptr;
            for (uint32_t k = 0; k < a.c.nops; ++k) {
                const uint32_t op = ld_const(a.c.ops, DF_WORDS * k), w1 = ld_const(a.c.ops, DF_WORDS * k + 1);
                const uint32_t code = scan_code(op), l = scan_level(op), g = scan_group(op);
                if (code == DF_F)
                    rater_op<DF_F>(sf, N, l, g);
                else if (code == DF_G)
                    rater_op<DF_G>(sf, N, l, g);
                else if (code == DF_COMB)
                    rater_op<DF_COMB>(sf, N, l, g);
                else
                    leaf8_op(sf, N, l, g, scan_flags(op), w1, ls, relw);
            }
            // the sign bits of the decoded words, packed; re-encoded for a non-systematic plan
            for (uint32_t q = 0; q < W; ++q) {
                uint32_t bits = 0;
                for (uint32_t j = 0; j < 32 && j < N; j += 4) {
                    const Vec<4> x = ldv<4>(sf, BITS + 32 * q + j);
#pragma unroll
                    for (uint32_t k = 0; k < 4; ++k)
                        bits |= (fbits(x.v[k]) >> 31) << (j + k);
                }
                row[q << 6] = bits;
            }
            if (!a.systematic) {
                for (uint32_t q = 0; q < W; ++q)
                    row[q << 6] = transform_word(row[q << 6], N);
                for (uint32_t d = 1; d < W; d <<= 1)
                    for (uint32_t q = 0; q < W; ++q)
                        if (!(q & d))
                            row[q << 6] ^= row[(q + d) << 6];
            }
            const bool pass_ok = detector_syndrome(row, W, a.c.crc_c0, a.c.crc_bits, a.c.crc_rows) == 0;
            const bool fin = !done && (pass_ok || run == TL); // this lane's last trial
            if (fin) {
                store_info_bytes(row, a.c.info_pos, K, a.c.kb, a.c.info + frame * a.c.kb);
                if (a.c.ok)
                    a.c.ok[frame] = pass_ok ? 1 : 0;
                if (a.ntrials)
                    a.ntrials[frame] = (uint8_t)run;
            }
            const uint64_t finm = ballot(fin);
            if (a.bits && finm) // the decoded words of the lanes that finish here
                rows_out(tile, sf, BITS, a.bits, frame0, nfr, N, T, lane, finm);
            done = done || pass_ok;
            if (run == TL || ballot(!done) == 0)
                break;
            // ---- Manager::decode: the first pass's order and the depth-0 entries ----
            if (run == 1) {
                float v0, v1;
                uint32_t i0, i1;
                next_weakest(rel, K, -__builtin_inff(), 0, v0, i0); // reliabilities are >= 0
                next_weakest(rel, K, v0, i0, v1, i1);
                ord1 = i1;
                *wordp(ent, 0) = ubits(entry0(i0, 0));
                if (TL > 1)
                    *wordp(ent, 1) = ubits(entry0(i0, 1));
                // nodeRank n = 1, 2, ...: (the n-th weakest, option 1) while the loop condition holds
                uint32_t n = 1;
                bool going = true;
                float vn = v1;
                uint32_t in_ = i1;
                ecount = 2;
                for (; n + 1 < TL; ++n) { // mConfigList.size() = n + 1 < trial limit
                    going = going && (n < TL * 2u / 3u || (double)vn < log9);
                    if (ballot(going) == 0)
                        break;
                    if (going) {
                        *wordp(ent, n + 1) = ubits(entry0(in_, 1));
                        ecount = n + 2;
                    }
                    float vv;
                    uint32_t ii;
                    next_weakest(rel, K, vn, in_, vv, ii);
                    vn = vv;
                    in_ = ii;
                }
                qsize = ecount;
            }
            // ---- Manager::decodeNext: pop entry run - 1, push its children, configure entry run ----
            {
                const uint32_t e = fbits(*wordp(ent, run - 1));
                qsize -= 1;
                if (qsize < TL) {
                    uint32_t c0 = DF_E_DEEPER, c1 = DF_E_DEEPER;
                    if (!(e & (DF_E_DEPTH1 | DF_E_DEEPER))) {
                        const uint32_t wk = run == 1 ? ord1 : ls.besti;
                        c0 = (e & (0xfffu | DF_E_OPT0)) | ((wk & 0xfffu) << 12) | DF_E_DEPTH1;
                        c1 = c0 | DF_E_OPT1;
                    }
                    if (ecount < TL)
                        *wordp(ent, ecount) = ubits(c0);
                    if (ecount + 1 < TL)
                        *wordp(ent, ecount + 1) = ubits(c1);
                    ecount += 2;
                    qsize += 2;
                }
                const uint32_t nx = fbits(*wordp(ent, run));
                const uint32_t n0 = nx & 0xfffu, n1 = (nx >> 12) & 0xfffu;
                ls.f0 = (nx & DF_E_OPT0) ? n0 : NO_LEAF;
                ls.f1 = (nx & DF_E_OPT1) ? n1 : NO_LEAF;
                ls.excl = n0;
            }
        }
    }
}

} // namespace

uint64_t depthfirst_wave_cap(uint32_t N, uint32_t slab_floats)
{
    return lane_wave_cap(depthfirst_kernel, lane_lds_bytes(N, true), 256ull * slab_floats);
}

int launch_depthfirst(const DepthFirstArgs& a, hipStream_t stream)
{
    return lane_launch(depthfirst_kernel, a, lane_lds_bytes(a.c.N, true), stream);
}

} // namespace pcg
