// channel_kernel.hip -- the simulator's transmission chain past BPSK-AWGN, one launch per batch:
//
//   modulate     Modulation::Ask::modulate       (ask.cpp:49-81), constants of setBitsPerSymbol
//   transmit     Transmission::Awgn / Rayleigh   (awgn.cpp:38-43, rayleigh.cpp:76-112,
//                                                 Random::Generator::getRayleighDist, random.cpp:92-104)
//   demodulate   Modulation::Ask::demodulate     (ask.cpp:83-101)
//   scale        Transmission::Scale             (scale.cpp)
//
// F x n/8 packed code bytes in (MSB-first, as pcg_encode writes them), F x n floats out.  With
// b bits per symbol a frame has S = ceil(n / b) symbols; bits past n count as 0.  Everything is
// fp32 with separate multiplies and adds (-ffp-contract=off).
//
// Noise is a pure function of (seed, frame, symbol): symbol j of frame f takes Box-Muller output
// j & 3 of Philox4x32-10 with key = seed and counter (4 (j >> 2), f_lo, f_hi, tag):
//
//   tag 0xA96   the additive noise g -- bpsk_awgn_kernel's counter, uniform mapping and expression
//               order, so at b = 1 on AWGN the received symbols are that kernel's bit for bit
//   tag 0xA97   g1, the fading's in-phase normal
//   tag 0xA98   g2, the fading's quadrature normal          h = sqrtf(g1 g1 + g2 g2)
//
// Thread t makes the four consecutive output floats 4t .. 4t+3 of the batch (one 16-byte store),
// like bpsk_awgn_kernel.  They belong to four symbols at b = 1, two at b = 2 and 3, and one or two
// above.  The division by b is a compile-time constant: the launch dispatches over b, and above 4
// bits per symbol also over who makes a symbol (shares_symbols below).
#include "frames.hpp"
#include "philox.hpp"
#include "wave.hpp"

#include <hip/hip_runtime.h>

namespace pcg {

namespace {

constexpr int kBlock = 256;
constexpr uint32_t kTagNoise = 0xA96u, kTagFadeRe = 0xA97u, kTagFadeIm = 0xA98u;

uint32_t grid_for(uint64_t items, uint32_t per_block)
{
    uint64_t g = (items + per_block - 1) / per_block;
    if (g > 65536u * 8u)
        g = 65536u * 8u; // grid-stride beyond this, as in frames_kernel.hip
    return (uint32_t)(g ? g : 1);
}

// One Box-Muller pair: radius and the two trigonometric factors; the normals are r * c and r * s.
struct Pair {
    float r, s, c;
};

__device__ __forceinline__ Pair box_muller(uint32_t a, uint32_t b)
{
    const float u1 = ((float)(a >> 8) + 1.0f) * (1.0f / 16777216.0f); // (0, 1]
    const float u2 = (float)(b >> 8) * (1.0f / 16777216.0f);          // [0, 1)
    Pair p;
    p.r = sqrtf(-2.0f * logf(u1));
    sincospif(2.0f * u2, &p.s, &p.c);
    return p;
}

struct Rng {
    uint32_t f_lo, f_hi, k0, k1;
};

// the pair that serves symbols 2p and 2p + 1
__device__ __forceinline__ Pair symbol_pair(const Rng& g, uint32_t p, uint32_t tag)
{
    const U4 r = philox(U4{(p >> 1) << 2, g.f_lo, g.f_hi, tag}, g.k0, g.k1);
    return (p & 1u) ? box_muller(r.z, r.w) : box_muller(r.x, r.y);
}

// the three pairs a symbol's channel draws from
template <bool RAY>
struct Draw {
    Pair n, re, im;
};

template <bool RAY>
__device__ __forceinline__ Draw<RAY> draw_pair(const Rng& g, uint32_t p, bool noisy)
{
    Draw<RAY> d{};
    if (noisy)
        d.n = symbol_pair(g, p, kTagNoise);
    if constexpr (RAY) {
        d.re = symbol_pair(g, p, kTagFadeRe);
        d.im = symbol_pair(g, p, kTagFadeIm);
    }
    return d;
}

// y = x h + sigma g for symbol j out of its pair's draw
template <bool RAY>
__device__ __forceinline__ float transmit(float x, const Draw<RAY>& d, uint32_t j, float sigma, bool noisy)
{
    const bool odd = j & 1u;
    if constexpr (RAY) {
        const float g1 = d.re.r * (odd ? d.re.s : d.re.c);
        const float g2 = d.im.r * (odd ? d.im.s : d.im.c);
        x = x * sqrtf(g1 * g1 + g2 * g2);
    }
    if (noisy)
        x += sigma * d.n.r * (odd ? d.n.s : d.n.c);
    return x;
}

// the B code bits from position p on, first bit at the top; bytes past the row read as 0
template <int B>
__device__ __forceinline__ uint32_t symbol_bits(const uint8_t* __restrict__ row, uint32_t nb, uint32_t p)
{
    constexpr int kBytes = (B + 14) / 8; // 8 kBytes >= 7 + B
    uint32_t w = 0;
#pragma unroll
    for (int k = 0; k < kBytes; ++k) {
        const uint32_t idx = (p >> 3) + k;
        w = (w << 8) | (idx < nb ? (uint32_t)row[idx] : 0u);
    }
    return (w >> (8 * kBytes - (p & 7u) - B)) & ((1u << B) - 1u);
}

// Ask::modulate's level of one symbol.  The reference runs m *= +-1; s = 2 s + m over the bits:
// s = sum_t (1 - 2 c_t) 2^(B-1-t) with c_t the parity of bits 0..t, i.e. (2^B - 1) - 2 C where C
// is the prefix XOR of the symbol's bits.  Every intermediate of the float recurrence is an
// integer below 2^17, so the integer form gives the same float.
template <int B>
__device__ __forceinline__ float ask_level(uint32_t v)
{
    uint32_t c = v;
    if constexpr (B > 1) c ^= c >> 1;
    if constexpr (B > 2) c ^= c >> 2;
    if constexpr (B > 4) c ^= c >> 4;
    if constexpr (B > 8) c ^= c >> 8;
    return (float)((int)((1u << B) - 1u) - 2 * (int)c);
}

struct ChannelArgs {
    const uint8_t* code;
    uint64_t F;
    uint32_t n;
    float sigma, gain, nm, pn;
    uint64_t seed;
    float* out;
    float* symbols;
};

template <int B, bool RAY, bool SHARE>
__global__ void __launch_bounds__(kBlock) ask_channel_kernel(ChannelArgs a)
{
    const uint32_t q = a.n >> 2, nb = a.n >> 3;
    const uint32_t S = (a.n + B - 1) / B;
    const uint64_t total = a.F * q;
    const bool noisy = a.sigma > 0.0f;
    for (uint64_t t = (uint64_t)blockIdx.x * kBlock + threadIdx.x; t < total; t += (uint64_t)gridDim.x * kBlock) {
        const uint64_t f = t / q;
        const uint32_t i = (uint32_t)(t - f * q) << 2;
        const uint8_t* row = a.code + f * nb;
        const Rng g{(uint32_t)f, (uint32_t)(f >> 32), (uint32_t)a.seed, (uint32_t)(a.seed >> 32)};
        float o[4];
        if constexpr (B == 1) {
            // four symbols, one Philox block per tag
            const uint8_t byte = row[i >> 3];
            float y[4];
#pragma unroll
            for (int k = 0; k < 4; ++k)
                y[k] = (((byte >> (7 - ((i + k) & 7))) & 1u) ? -1.0f : 1.0f) * a.pn;
            if constexpr (RAY) {
                const U4 re = philox(U4{i, g.f_lo, g.f_hi, kTagFadeRe}, g.k0, g.k1);
                const U4 im = philox(U4{i, g.f_lo, g.f_hi, kTagFadeIm}, g.k0, g.k1);
                const Pair ra = box_muller(re.x, re.y), rb = box_muller(re.z, re.w);
                const Pair ia = box_muller(im.x, im.y), ib = box_muller(im.z, im.w);
                const float g1[4] = {ra.r * ra.c, ra.r * ra.s, rb.r * rb.c, rb.r * rb.s};
                const float g2[4] = {ia.r * ia.c, ia.r * ia.s, ib.r * ib.c, ib.r * ib.s};
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    y[k] = y[k] * sqrtf(g1[k] * g1[k] + g2[k] * g2[k]);
            }
            if (noisy) {
                const U4 r = philox(U4{i, g.f_lo, g.f_hi, kTagNoise}, g.k0, g.k1);
                const Pair pa = box_muller(r.x, r.y), pb = box_muller(r.z, r.w);
                y[0] += a.sigma * pa.r * pa.c;
                y[1] += a.sigma * pa.r * pa.s;
                y[2] += a.sigma * pb.r * pb.c;
                y[3] += a.sigma * pb.r * pb.s;
            }
            if (a.symbols)
                *reinterpret_cast<float4*>(a.symbols + f * S + i) = make_float4(y[0], y[1], y[2], y[3]);
#pragma unroll
            for (int k = 0; k < 4; ++k)
                o[k] = y[k] * a.nm; // shift = 2^0 is never used: one bit per symbol
        } else {
            // bits i .. i+3 lie in symbols j0 and j1 <= j0 + 1
            const uint32_t j0 = i / B, j1 = (i + 3) / B;
            float y0, y1;
            if constexpr (SHARE) {
                // One lane per symbol.  n % 256 == 0, so the wave's 256 bits lie in one frame, in at
                // most 64 symbols (B >= 5): lane l makes symbol jbase + l and stores it, then every
                // lane fetches its two.  Waves enter and leave the loop whole (q % 64 == 0).
                const uint32_t lane = lane_id();
                const uint32_t ibase = i - 4u * lane;
                const uint32_t jbase = ibase / B, jm = jbase + lane;
                float ym = 0.0f;
                if (jm * B < ibase + 256u) {
                    const Draw<RAY> d = draw_pair<RAY>(g, jm >> 1, noisy);
                    ym = transmit<RAY>(ask_level<B>(symbol_bits<B>(row, nb, jm * B)) * a.pn, d, jm, a.sigma, noisy);
                    if (a.symbols && jm * B >= ibase) // a symbol is stored by the wave that holds its first bit
                        a.symbols[f * S + jm] = ym;
                }
                y0 = __shfl(ym, (int)(j0 - jbase), 64);
                y1 = __shfl(ym, (int)(j1 - jbase), 64);
            } else {
                // Every lane makes its own one or two symbols.
                const Draw<RAY> d0 = draw_pair<RAY>(g, j0 >> 1, noisy);
                y0 = transmit<RAY>(ask_level<B>(symbol_bits<B>(row, nb, j0 * B)) * a.pn, d0, j0, a.sigma, noisy);
                y1 = y0;
                if (B < 4 || j1 != j0) {
                    Draw<RAY> d1 = d0;
                    if (B != 2 && (j1 >> 1) != (j0 >> 1)) // b = 2: j0 is even, one pair serves both
                        d1 = draw_pair<RAY>(g, j1 >> 1, noisy);
                    y1 = transmit<RAY>(ask_level<B>(symbol_bits<B>(row, nb, j1 * B)) * a.pn, d1, j1, a.sigma, noisy);
                }
                if (a.symbols) {
                    // a symbol is stored by the thread that holds its first bit
                    if (j0 * B >= i)
                        a.symbols[f * S + j0] = y0;
                    if (j1 != j0)
                        a.symbols[f * S + j1] = y1;
                }
            }
            // demodulate: out[k] = a; a = |a| - shift; shift /= 2 along a symbol's bits.  The first
            // of the four bits walks there from its symbol's start, the others continue from their
            // left neighbour or start symbol j1.
            uint32_t pos = i - j0 * B;
            float amp = y0 * a.nm;
            {
                float shift = (float)(1u << (B - 1));
#pragma unroll
                for (int s = 0; s < B - 1; ++s) {
                    if ((uint32_t)s < pos)
                        amp = fabsf(amp) - shift;
                    shift *= 0.5f;
                }
            }
            o[0] = amp;
#pragma unroll
            for (int k = 1; k < 4; ++k) {
                if (++pos == (uint32_t)B) { // (i + k) is j1's first bit
                    pos = 0;
                    amp = y1 * a.nm;
                } else {
                    amp = fabsf(amp) - __uint_as_float((127u + (uint32_t)B - pos) << 23); // 2^(B - pos)
                }
                o[k] = amp;
            }
        }
        *reinterpret_cast<float4*>(a.out + f * a.n + i) =
            make_float4(o[0] * a.gain, o[1] * a.gain, o[2] * a.gain, o[3] * a.gain);
    }
}

// Above 4 bits per symbol several lanes need the same symbol.  Measured on 2^16 x 1024 bits at b = 10
// (DESIGN.md (f)): one lane per symbol with a cross-lane fetch 0.110 ms, every lane recomputing
// 0.128 ms, so the exchange is used where it applies: b >= 5 that is no multiple of 4 (at 4, 8, 12
// and 16 the four bits never straddle two symbols and a lane makes exactly one) and n % 256 == 0.
constexpr bool shares_symbols(int b) { return b >= 5 && b % 4 != 0; }

template <bool RAY>
void launch_for_bits(uint32_t b, bool whole_waves, dim3 grid, hipStream_t s, const ChannelArgs& a)
{
    switch (b) {
#define PCG_ASK_CASE(B)                                                                               \
    case B:                                                                                           \
        if (shares_symbols(B) && whole_waves)                                                         \
            hipLaunchKernelGGL((ask_channel_kernel<B, RAY, shares_symbols(B)>), grid, dim3(kBlock), 0, s, a); \
        else                                                                                          \
            hipLaunchKernelGGL((ask_channel_kernel<B, RAY, false>), grid, dim3(kBlock), 0, s, a);     \
        break;
        PCG_ASK_CASE(1) PCG_ASK_CASE(2) PCG_ASK_CASE(3) PCG_ASK_CASE(4) PCG_ASK_CASE(5) PCG_ASK_CASE(6)
        PCG_ASK_CASE(7) PCG_ASK_CASE(8) PCG_ASK_CASE(9) PCG_ASK_CASE(10) PCG_ASK_CASE(11) PCG_ASK_CASE(12)
        PCG_ASK_CASE(13) PCG_ASK_CASE(14) PCG_ASK_CASE(15) PCG_ASK_CASE(16)
#undef PCG_ASK_CASE
    }
}

} // namespace

int launch_ask_channel(const uint8_t* code, uint64_t F, uint32_t n, uint32_t bits_per_symbol, bool rayleigh,
                       float sigma, float gain, float nm, float pn, uint64_t seed, float* out, float* symbols,
                       hipStream_t s)
{
    if (F == 0)
        return 0;
    const ChannelArgs a{code, F, n, sigma, gain, nm, pn, seed, out, symbols};
    const dim3 grid(grid_for(F * (n / 4), kBlock));
    const bool whole_waves = n % 256 == 0; // a wave's 64 x 4 bits in one frame
    if (rayleigh)
        launch_for_bits<true>(bits_per_symbol, whole_waves, grid, s, a);
    else
        launch_for_bits<false>(bits_per_symbol, whole_waves, grid, s, a);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

} // namespace pcg
