// fsscan.hpp -- the Fast-SSCAN soft-output decoder (PolarCode::Decoding::FastSscanFloat,
// fastsscan_float.cpp): schedule words, kernel arguments and launch interface shared by plan.cpp,
// capi.cpp and fsscan_kernel.hip.  What it has in common with SCAN (the word format, polar_f)
// comes from scan.hpp / wave.hpp.
#pragma once
#include "scan.hpp"

namespace pcg {

// One op = three 32-bit words.  Word 0 is a scan.hpp word (code | level << 4 | group << 8 |
// flags << 24): (level, group) name the node, level 0 is the root, a node of level l holds
// N >> l values in natural order (the first half is the left child's); the kernel reads code,
// level and flags, the group only names the node when a schedule is dumped.  Word 1 is the slab
// offset (floats per lane) of the right child's message, word 2 that of the node's own message.
enum FsscanOp : uint32_t {
    FSS_LEFT = 1,  // RateR: left child's input  = F(er + b, a)            fastsscan_float.cpp:142-143
    FSS_RIGHT = 2, // RateR: right child's input = F(el, a) + b            :149-150
    FSS_OUT = 3,   // RateR: message = ( F(el, er + b) | er + F(el, a) )   :157-161
    FSS_REP = 4,   // Repetition: message[i] = sum - in[i]                 :202-223
    FSS_TWO = 5,   // TwoBit: message = (in[1], in[0])                     :231-235
    FSS_CONST = 6, // a root that is a Zero (+inf) or One (+0) node: its message, written once
};
// a child that is a constant node is an operand of its parent's expressions
constexpr uint32_t FSS_L_ZERO = 1u; // left child is a Zero node: el = +inf
constexpr uint32_t FSS_L_ONE = 2u;  // left child is a One node:  el = +0
constexpr uint32_t FSS_R_ZERO = 4u; // right child is a Zero node: er = +inf
constexpr uint32_t FSS_R_ONE = 8u;  // right child is a One node:  er = +0
constexpr uint32_t FSS_WORDS = 3;

// Slab of one lane, in floats: IN at offset 0 (the inputs of the nodes of each level, level l at
// fsscan_lvl(N, l); level 0 holds the channel LLRs), EL (the messages of the root and of the left
// children, same offsets), then the messages of the right children, which alone live across
// passes (offsets assigned by plan.cpp fsscan_emit, multiples of 4).
constexpr inline uint32_t fsscan_lvl(uint32_t N, uint32_t l) { return 2u * (N - (N >> l)); }
constexpr inline uint32_t fsscan_el(uint32_t N) { return 2u * N; }
constexpr inline uint32_t fsscan_er(uint32_t N) { return 4u * N; }

struct FsscanArgs {
    LaneArgs c;       // ops: the schedule of one pass, FSS_WORDS words per op
    uint32_t trials;  // trial limit, 1 .. 255
    int forced;       // run exactly `trials` passes; the check only after the last
    float* soft;      // F x N or null
    uint8_t* ntrials; // F or null: passes run
};

// The Fast-SSCAN plan: validation, info positions and detector model as build_plan; `ops` =
// FsscanOp words of one pass, node_types = the pre-order census of createDecoder's node kinds
// (FSS_NODE_*), *slab_floats = the floats of state one codeword keeps.
enum FsscanNode : int { FSS_NODE_RATER = 0, FSS_NODE_ZERO = 1, FSS_NODE_ONE = 2, FSS_NODE_TWO = 3, FSS_NODE_REP = 4 };
int build_fsscan_plan(PlanHost& p, uint32_t N, const uint32_t* frozen, uint32_t nf, int systematic, int crc_kind,
                      uint32_t* slab_floats, std::string* err);

uint64_t fsscan_wave_cap(uint32_t N, uint32_t slab_floats);
int launch_fsscan(const FsscanArgs& a, hipStream_t stream);

} // namespace pcg
