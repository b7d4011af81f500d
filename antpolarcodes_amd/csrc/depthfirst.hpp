// depthfirst.hpp -- the SC-Flip decoder (PolarCode::Decoding::DepthFirst, depth_first.cpp):
// schedule words, kernel arguments and launch interface shared by plan.cpp, capi.cpp and
// depthfirst_kernel.hip.  The word format and polar_f come from scan.hpp / wave.hpp.
#pragma once
#include "scan.hpp"

namespace pcg {

// One op = two 32-bit words.  Word 0 is a scan.hpp word (code | level << 4 | group << 8 |
// flags << 24): (level, group) name the node, level 0 is the root, a node of level l holds
// n = N >> l values in natural order at positions [group * n, group * n + n).  For DF_LEAF8 the
// flags are the frozen mask of the node's eight leaves (bit i = leaf i is frozen) and word 1 is
// the rank, among the K information leaves, of its first leaf; else word 1 is 0.
enum DepthFirstOp : uint32_t {
    DF_F = 1,     // RateR: left child's input  = F(a, b)                     depth_first.cpp:279
    DF_G = 2,     // RateR: right child's input = (a ^ sign(left bits)) + b   :281
    DF_COMB = 3,  // RateR: bits = (left ^ right | right), whole words        :283
    DF_LEAF8 = 4, // a size-8 subtree (ShortRateR nodes over single-bit leaves) in registers :307-315
};
constexpr uint32_t DF_WORDS = 2;
constexpr uint32_t DF_MAX_TRIALS = 255;

// Slab of one lane, in 32-bit words: the inputs of the nodes of each level (level l at
// df_lvl(N, l); level 0 holds the channel LLRs), the N decoded words of the codeword, the K
// first-pass reliabilities (padded to a multiple of 4), and the search entries of the trials.
constexpr inline uint32_t df_lvl(uint32_t N, uint32_t l) { return 2u * (N - (N >> l)); }
constexpr inline uint32_t df_bits(uint32_t N) { return 2u * N; }
constexpr inline uint32_t df_rel(uint32_t N) { return 3u * N; }
constexpr inline uint32_t df_ent(uint32_t N, uint32_t K) { return 3u * N + ((K + 3u) & ~3u); }
constexpr inline uint32_t df_slab_floats(uint32_t N, uint32_t K) { return df_ent(N, K) + DF_MAX_TRIALS + 1u; }

// A search entry (one configuration of the reference's queue, as far as a trial can reach it):
// prefix leaves n0, n1 (information ranks, 12 bits each), their options, and the depth.
constexpr uint32_t DF_E_OPT0 = 1u << 24, DF_E_OPT1 = 1u << 25, DF_E_DEPTH1 = 1u << 26, DF_E_DEEPER = 1u << 27;

struct DepthFirstArgs {
    LaneArgs c;       // ops: the schedule of one root decode, DF_WORDS words per op
    uint32_t trials;  // trial limit, 1 .. 255
    int systematic;
    uint32_t* bits;   // F x N decoded words or null
    uint8_t* ntrials; // F or null: trials run
};

// The SC-Flip plan: validation, info positions and detector model as build_plan; `ops` =
// DepthFirstOp words of one root decode, node_count = all nodes of the unpruned tree.
// -1 bad argument (K < max(trial_limit, 2) included), -4 N above SCAN_MAX_N.
int build_depthfirst_plan(PlanHost& p, uint32_t N, uint32_t trial_limit, const uint32_t* frozen, uint32_t nf,
                          int systematic, int crc_kind, uint32_t* slab_floats, std::string* err);

uint64_t depthfirst_wave_cap(uint32_t N, uint32_t slab_floats);
int launch_depthfirst(const DepthFirstArgs& a, hipStream_t stream);

} // namespace pcg
