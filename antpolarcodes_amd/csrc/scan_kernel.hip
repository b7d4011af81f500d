// scan_kernel.hip -- batched SCAN soft-output polar decoding on CDNA4 (gfx950).
//
// The reference's PolarCode::Decoding::Scan (scan.cpp, after Fayyaz and Barry) with lane = one
// codeword: a wave decodes 64 frames at once and walks the plan's schedule (plan.cpp scan_emit:
// the recursion updatellrmap / updatebitmap of scan.cpp:80-210 written out in decode order)
// uniformly, every lane running the reference's scalar expressions on its own state.  Every
// value has one fixed fp32 expression, so the outputs equal the reference's bit for bit.
//
// Per wave, in a global slab of float2 units (unit u of lane l at float2 [u * 64 + l]: a
// wave-wide unit access is one contiguous 512 B; a node's values 2v, 2v+1 are unit v):
//   L  N units    LLRs toward the leaves, level l at N - (N >> l)          (mLlr)
//   E  N units    messages toward the root of the even groups, same offsets (mEven)
//   O  (log2N - 1) N/4 units  the same of the odd groups of levels 1 .. log2N-1 (mOdd)
//   S  N/2 units  non-systematic plans: the per-leaf outputs             (mSystematicOutput)
// Leaf-level values never reach memory: a size-2 node runs in registers (SCAN_LEAF2), and the
// leaf messages are constants (+inf frozen, +0 information).  Nothing is zeroed: L and E are
// written before they are read in every iteration, and the first iteration takes O as the
// reference's initial +0.
//
// All-frozen subtrees are pruned (DESIGN.md "SCAN"): their messages toward the root are +inf for
// finite LLRs, which the ops of their parents take as constants (SCAN_EINF / SCAN_OINF) -- in the
// first iteration a right all-frozen child's message is still the initial +0 where its left
// sibling reads it, as in the reference.
//
// Frame rows in and out through the transpose tile, the detector syndrome, the information bytes
// and the launch are lane_frame.hpp's; the bit reversal between a row and the slab stays here.
#include "lane_frame.hpp"

namespace pcg {

namespace {

PCG_DEV uint32_t bitrev(uint32_t v, uint32_t nbits) { return __builtin_bitreverse32(v) >> (32u - nbits); }

struct ScanLayout {
    uint32_t L, E, O, S, units; // float2-unit offsets in a wave's slab; units per wave
};
__host__ __device__ inline ScanLayout scan_layout(uint32_t N, uint32_t n, int systematic)
{
    ScanLayout y;
    y.L = 0;
    y.E = N;
    y.O = 2 * N;
    y.S = y.O + (n - 1) * (N / 4);
    y.units = y.S + (systematic ? 0u : N / 2);
    return y;
}

struct Wave {
    float2* s; // slab + lane
    uint32_t N, n;
    ScanLayout ly;
    PCG_DEV float2* lvl(uint32_t base, uint32_t l) const { return s + (uint64_t)(base + N - (N >> l)) * 64u; }
    // O of the odd group g at level l (1 <= l <= n-1)
    PCG_DEV float2* odd(uint32_t l, uint32_t g) const
    {
        return s + (uint64_t)(ly.O + (l - 1) * (N / 4) + ((g - 1) >> 1) * ((N >> l) / 2)) * 64u;
    }
    // where node (l, g) keeps its message toward the root
    PCG_DEV float2* up(uint32_t l, uint32_t g) const { return (g & 1u) ? odd(l, g) : lvl(ly.E, l); }
};

PCG_DEV float2 ldu(const float2* b, uint32_t u) { return b[u << 6]; }
PCG_DEV void stu(float2* b, uint32_t u, const float2& v) { b[u << 6] = v; }

// the three internal ops over child units [v0, v0 + B)
template <uint32_t CODE, uint32_t B>
PCG_DEV void node_units(const float2* P, const float2* Ec, const float2* Oc, float2* D, uint32_t v0, bool e_ld,
                        float ec, bool o_ld, float oc)
{
    float2 p0[B], p1[B], e[B], o[B];
#pragma unroll
    for (uint32_t q = 0; q < B; ++q) {
        p0[q] = ldu(P, 2 * (v0 + q));
        p1[q] = ldu(P, 2 * (v0 + q) + 1);
        if (CODE != SCAN_DOWN_L)
            e[q] = e_ld ? ldu(Ec, v0 + q) : make_float2(ec, ec);
        if (CODE != SCAN_DOWN_R)
            o[q] = o_ld ? ldu(Oc, v0 + q) : make_float2(oc, oc);
    }
#pragma unroll
    for (uint32_t q = 0; q < B; ++q) {
        if (CODE == SCAN_DOWN_L) { // L = F(L[2i], L[2i+1] + O)                    scan.cpp:110-113
            stu(D, v0 + q, make_float2(polar_f(p0[q].x, p0[q].y + o[q].x), polar_f(p1[q].x, p1[q].y + o[q].y)));
        } else if (CODE == SCAN_DOWN_R) { // L = L[2i+1] + F(L[2i], E)               scan.cpp:92-96
            stu(D, v0 + q, make_float2(p0[q].y + polar_f(p0[q].x, e[q].x), p1[q].y + polar_f(p1[q].x, e[q].y)));
        } else { // U[2i] = F(E, O + L[2i+1]), U[2i+1] = O + F(E, L[2i])              scan.cpp:135-157, 172-193
            stu(D, 2 * (v0 + q),
                make_float2(polar_f(e[q].x, o[q].x + p0[q].y), o[q].x + polar_f(e[q].x, p0[q].x)));
            stu(D, 2 * (v0 + q) + 1,
                make_float2(polar_f(e[q].y, o[q].y + p1[q].y), o[q].y + polar_f(e[q].y, p1[q].x)));
        }
    }
}

template <uint32_t CODE>
PCG_DEV void node_op(const Wave& w, uint32_t l, uint32_t g, uint32_t flags, bool first)
{
    const float inf = __builtin_inff();
    const uint32_t nu = w.N >> (l + 2); // units of a child
    const float2* P = w.lvl(w.ly.L, l);
    const float2* Ec = w.lvl(w.ly.E, l + 1);
    const float2* Oc = w.odd(l + 1, 2 * g + 1);
    float2* D = CODE == SCAN_UP ? w.up(l, g) : w.lvl(w.ly.L, l + 1);
    const bool e_ld = !(flags & SCAN_EINF);
    // the right child's message: what the previous iteration left (the initial +0 in the first
    // one) where the left child's LLRs are computed, this iteration's afterwards
    const bool o_ld = !(flags & SCAN_OINF) && !(CODE == SCAN_DOWN_L && first);
    const float oc = (CODE == SCAN_DOWN_L && first) ? 0.0f : inf;
    uint32_t v = 0;
    for (; v + 4 <= nu; v += 4)
        node_units<CODE, 4>(P, Ec, Oc, D, v, e_ld, inf, o_ld, oc);
    for (; v < nu; ++v)
        node_units<CODE, 1>(P, Ec, Oc, D, v, e_ld, inf, o_ld, oc);
}

__global__ void __launch_bounds__(64) scan_kernel(ScanArgs a)
{
    extern __shared__ uint32_t smem_scan[];
    uint32_t* tile = smem_scan;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t N = a.c.N, n = a.log2N;
    const uint32_t T = N < TILE ? N : TILE;
    const uint32_t W = N >= 32 ? N / 32 : 1u;
    uint32_t* row = smem_scan + TILE * TILE_STRIDE + lane; // own sign-bit row, word q at [q * 64]
    Wave w;
    w.N = N;
    w.n = n;
    w.ly = scan_layout(N, n, a.systematic);
    w.s = reinterpret_cast<float2*>(a.c.slab) + (uint64_t)blockIdx.x * w.ly.units * 64u + lane;
    float* sf = reinterpret_cast<float*>(w.s); // element e of unit u at sf[u * 128 + e]
    const float inf = __builtin_inff();
    const uint64_t ngroups = (a.c.F + 63) / 64;
    for (uint64_t grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {
        const uint64_t frame0 = grp * 64, frame = frame0 + lane;
        const uint32_t nfr = a.c.F - frame0 < 64 ? (uint32_t)(a.c.F - frame0) : 64u;
        // channel LLRs into level 0, bit-reversed (scan.cpp:229-233), transposed through LDS
        for (uint32_t c = 0; c < N / T; ++c) {
            tile_in(tile, a.c.llr, frame0, nfr, N, c, T, lane);
            for (uint32_t j = 0; j < T; ++j) {
                const uint32_t r = bitrev(c * T + j, n);
                sf[(uint64_t)(w.ly.L + (r >> 1)) * 128u + (r & 1u)] = ubits(tile[lane * TILE_STRIDE + j]);
            }
            wsync();
        }
        for (uint32_t it = 0; it < a.iters; ++it) {
            const bool first = it == 0;
            for (uint32_t k = 0; k < a.c.nops; ++k) {
                const uint32_t op = ld_const(a.c.ops, k);
                const uint32_t code = scan_code(op), l = scan_level(op), g = scan_group(op), fl = scan_flags(op);
                if (code == SCAN_DOWN_L) {
                    node_op<SCAN_DOWN_L>(w, l, g, fl, first);
                } else if (code == SCAN_DOWN_R) {
                    node_op<SCAN_DOWN_R>(w, l, g, fl, first);
                } else if (code == SCAN_UP) {
                    node_op<SCAN_UP>(w, l, g, fl, first);
                } else if (code == SCAN_LEAF2) {
                    // level n-1: L = (x, y); the leaves' messages are constants (scan.cpp:235-242, 259-270)
                    const float2 p = ldu(w.lvl(w.ly.L, l), 0);
                    const float el = (fl & SCAN_EINF) ? inf : 0.0f, ol = (fl & SCAN_OINF) ? inf : 0.0f;
                    if (!a.systematic) {
                        const float ll = polar_f(p.x, p.y + ol), lr = p.y + polar_f(p.x, el);
                        stu(w.s + (uint64_t)w.ly.S * 64u, g, make_float2(ll + el, lr + ol));
                    }
                    stu(w.up(l, g), 0, make_float2(polar_f(el, ol + p.y), ol + polar_f(el, p.x)));
                } else { // SCAN_FROZEN: the leaves' L + inf
                    const uint32_t nu = N >> (l + 1);
                    float2* S = w.s + (uint64_t)(w.ly.S + g * nu) * 64u;
                    for (uint32_t v = 0; v < nu; ++v)
                        stu(S, v, make_float2(inf, inf));
                }
            }
        }
        // outputs (scan.cpp:275-304), un-bit-reversed: the soft codeword with its sign bits, the
        // extrinsic channel information
        for (uint32_t c = 0; c < N / T; ++c) {
            uint32_t bits = 0;
            for (uint32_t j = 0; j < T; ++j) {
                const uint32_t r = bitrev(c * T + j, n);
                const uint64_t e = (uint64_t)(r >> 1) * 128u + (r & 1u);
                float v;
                if (a.systematic)
                    v = sf[(uint64_t)w.ly.L * 128u + e] + (a.iters ? sf[(uint64_t)w.ly.E * 128u + e] : 0.0f);
                else
                    v = a.iters ? sf[(uint64_t)w.ly.S * 128u + e] : 0.0f;
                bits |= (fbits(v) >> 31) << (j & 31u);
                if ((j & 31u) == 31u || j + 1 == T) {
                    row[((c * T + j) >> 5) << 6] = bits;
                    bits = 0;
                }
                if (a.soft)
                    tile[lane * TILE_STRIDE + j] = fbits(v);
            }
            if (a.soft)
                tile_out(tile, reinterpret_cast<uint32_t*>(a.soft), frame0, nfr, N, c, T, lane, ~0ull);
        }
        if (a.ext)
            for (uint32_t c = 0; c < N / T; ++c) {
                for (uint32_t j = 0; j < T; ++j) {
                    const uint32_t r = bitrev(c * T + j, n);
                    tile[lane * TILE_STRIDE + j] =
                        a.iters ? fbits(sf[(uint64_t)w.ly.E * 128u + (uint64_t)(r >> 1) * 128u + (r & 1u)]) : 0u;
                }
                tile_out(tile, reinterpret_cast<uint32_t*>(a.ext), frame0, nfr, N, c, T, lane, ~0ull);
            }
        // detector syndrome and info bytes from the sign bits
        const uint32_t syn = detector_syndrome(row, W, a.c.crc_c0, a.c.crc_bits, a.c.crc_rows);
        if (frame < a.c.F) {
            store_info_bytes(row, a.c.info_pos, a.c.K, a.c.kb, a.c.info + frame * a.c.kb);
            if (a.c.ok)
                a.c.ok[frame] = syn == 0 ? 1 : 0;
        }
    }
}

} // namespace

uint64_t scan_slab_floats(uint32_t N, int systematic)
{
    return 128ull * scan_layout(N, (uint32_t)__builtin_ctz(N), systematic).units;
}

uint64_t scan_wave_cap(uint32_t N, uint32_t slab_floats)
{
    return lane_wave_cap(scan_kernel, lane_lds_bytes(N, true), 256ull * slab_floats);
}

int launch_scan(const ScanArgs& a, hipStream_t stream)
{
    return lane_launch(scan_kernel, a, lane_lds_bytes(a.c.N, true), stream);
}

} // namespace pcg
