// errorlocator.hpp -- the genie-aided SC error locator (PolarCode::Decoding::ErrorLocator,
// errorlocator.cpp): kernel arguments and launch interface shared by plan.cpp, capi.cpp and
// errorlocator_kernel.hip.  The schedule is the SC-Flip decoder's (depthfirst.hpp: DF_* words,
// plan.cpp depthfirst_emit); polar_f / polar_g come from wave.hpp.
#pragma once
#include "depthfirst.hpp"

namespace pcg {

// What a launch does at the information leaves (fixed per launch); a frozen leaf outputs its
// desired value in every mode.
enum ErrorLocatorMode : uint32_t {
    EL_REFERENCE = 0, // setAsReferenceDecoder() + decode(): no comparison            errorlocator.cpp:216-217
    EL_CORRECT = 1,   // decode(): a leaf whose sign differs from its desired value's is replaced :219-222
    EL_FIRST = 2,     // decodeFindFirstError(): compare, never replace                :227-232
};

// Slab of one lane, in 32-bit words: the inputs of the nodes of each level (df_lvl; level 0 holds
// the channel LLRs), the N decoded words (df_bits), and the N desired values, each overwritten by
// its leaf's value once that leaf is done.
constexpr inline uint32_t el_des(uint32_t N) { return 3u * N; }
constexpr inline uint32_t el_slab_floats(uint32_t N) { return 4u * N; }

struct ErrorLocatorArgs {
    LaneArgs c;           // ops: the SC-Flip schedule of one root decode; no info, ok or detector
    const float* desired; // F x N desired leaf values, or null: +0 at information leaves, +inf at frozen ones
    uint32_t mode;        // ErrorLocatorMode
    float* u;             // F x N leaf values (getOutput) or null
    uint32_t* bits;       // F x N decoded words (getSoftCodeword) or null
    int32_t* first;       // F or null
    uint32_t* count;      // F or null
};

// The error-locator plan: build_depthfirst_plan's validation without the trial-limit rules (at
// least one information bit), its schedule and node count; no detector.
// -1 bad argument, -4 N above SCAN_MAX_N.
int build_errorlocator_plan(PlanHost& p, uint32_t N, const uint32_t* frozen, uint32_t nf, uint32_t* slab_floats,
                            std::string* err);

uint64_t errorlocator_wave_cap(uint32_t N, uint32_t slab_floats);
int launch_errorlocator(const ErrorLocatorArgs& a, hipStream_t stream);

} // namespace pcg
