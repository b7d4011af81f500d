// scan.hpp -- the SCAN soft-output decoder (PolarCode::Decoding::Scan, scan.cpp): schedule
// words, kernel arguments and launch interface shared by plan.cpp, capi.cpp and scan_kernel.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

namespace pcg {

// One op = one 32-bit word: code | level << 4 | group << 8 | flags << 24.  (level, group) name
// a node of the reference's tree: level 0 is the root (N values), group its index in the level
// (scan.cpp's `level` and `group`); a node of level l holds N >> l values.
enum ScanOp : uint32_t {
    SCAN_DOWN_L = 1, // L of the left child   (updatellrmap, even group, scan.cpp:109-124)
    SCAN_DOWN_R = 2, // L of the right child  (updatellrmap, odd group,  scan.cpp:90-107)
    SCAN_UP = 3,     // the node's message toward the root from its children's (updatebitmap :128-205)
    SCAN_LEAF2 = 4,  // a whole size-2 node in registers: both leaves and its upward message
    SCAN_FROZEN = 5, // non-systematic plans: the output of a pruned all-frozen subtree (+inf)
};
// DOWN_L / DOWN_R / UP: a child that is a pruned all-frozen subtree sends +inf; LEAF2: frozen leaves
constexpr uint32_t SCAN_EINF = 1u; // left child (LEAF2: left leaf frozen)
constexpr uint32_t SCAN_OINF = 2u; // right child (LEAF2: right leaf frozen)

constexpr inline uint32_t scan_code(uint32_t w) { return w & 0xfu; }
constexpr inline uint32_t scan_level(uint32_t w) { return (w >> 4) & 0xfu; }
constexpr inline uint32_t scan_group(uint32_t w) { return (w >> 8) & 0xffffu; }
constexpr inline uint32_t scan_flags(uint32_t w) { return w >> 24; }

constexpr uint32_t SCAN_MAX_N = 4096;

// What every lane = codeword kernel is given (lane_frame.hpp); the first member `c` of the
// kernels' argument structs.  The error locator has no detector and no information bytes.
struct LaneArgs {
    const float* llr; // F x N channel LLRs (device)
    uint64_t F;
    const uint32_t* ops; // flattened schedule (device)
    uint32_t nops;
    uint32_t N, K, kb;
    const uint16_t* info_pos; // K info positions (device)
    uint32_t crc_c0;
    uint32_t crc_bits;
    const uint32_t* crc_rows; // as KernelArgs::crc_rows
    uint8_t* info;        // F x kb
    uint8_t* ok;          // F or null
    float* slab;          // units x 64 x slab_floats
    uint32_t slab_floats; // words per lane (a multiple of 4)
    uint32_t units;       // grid size (persistent waves)
};

struct ScanArgs {
    LaneArgs c; // ops: ScanOp words of one iteration; slab_floats = scan_slab_floats / 64
    uint32_t log2N;
    uint32_t iters;
    int systematic;
    float* soft; // F x N or null
    float* ext;  // F x N or null
};

// The SCAN plan: validation, info positions and detector model as build_plan, `ops` = ScanOp
// words of one iteration (plan.cpp scan_emit).  -1 bad argument, -4 N above SCAN_MAX_N.
struct PlanHost;
int build_scan_plan(PlanHost& p, uint32_t N, const uint32_t* frozen, uint32_t nf, int systematic, int crc_kind,
                    std::string* err);

// floats of global state one wave (64 codewords) keeps
uint64_t scan_slab_floats(uint32_t N, int systematic);
uint64_t scan_wave_cap(uint32_t N, uint32_t slab_floats); // slab_floats: per lane, as LaneArgs
int launch_scan(const ScanArgs& a, hipStream_t stream);

} // namespace pcg
