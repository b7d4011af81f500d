/* -*- c++ -*- */
// PolarCode::Decoding::ErrorLocator -- drop-in for the reference's genie-aided SC error locator
// (include/polarcode/decoding/errorlocator.h, src/polarcode/decoding/errorlocator.cpp), the
// decoder behind its `errorlocator` tool ("bad bit finder"); on the MI355X
// (errorlocator_kernel.hip through pcg_plan_create_errorlocator of include/pcg.h).
//
// Plain successive cancellation down to single bits.  A bit outputs its LLR or, when replaced, its
// desired value; frozen bits always output their desired value (+inf unless setDesiredOutput gave
// another), information bits (desired +0.0f by default) are replaced by decode() when the sign of
// their LLR differs from the sign of their desired value: the genie.  firstError() is the index of
// the first bit replaced and correctionCount() how many were.  After setAsReferenceDecoder(),
// decode() compares nothing (and leaves firstError() / correctionCount() alone).  The reference
// decodes once per correction; this class decodes once (SC is causal, see include/pcg.h) and
// every value equals the reference's bit for bit for finite LLRs whose sums stay finite.
//
// The reference's members keep their names and meanings: the constructor, decode() (always true),
// initialize, clear, decodeFindFirstError, getOutput, setDesiredOutput, setAsReferenceDecoder,
// firstError, correctionCount, and Decoder's setSignal / getSoftCodeword.  The node classes
// (ErrorLocatorNodes) and pushBit are the reference's internals and are not reproduced.  The
// decoder produces no information bytes.  New: locateBatch() / locateBatchDevice() for F frames
// per call.  Construction validates on a host-only plan and needs no GPU.
#ifndef PCA_DEC_ERRLOC_H
#define PCA_DEC_ERRLOC_H

#include <polarcode/decoding/decoder.h>
#include <vector>

namespace PolarCode {
namespace Decoding {

class ErrorLocator : public Decoder
{
    int mDevice;
    pcg_plan* mPlan = nullptr;
    std::vector<float> mDesired; // empty: the defaults (+0 at information bits, +inf at frozen bits)
    std::vector<float> mOutput;
    int mFirstError = -1;
    int mCorrectionCount = 0;
    bool mIsReferenceDecoder = false;

    void ensurePlan();
    void releasePlan();
    int run(int mode);

public:
    /// What a locateBatch call does at the information bits (PCG_EL_* of include/pcg.h).
    enum Mode { Reference = 0, Correct = 1, First = 2 };

    ErrorLocator(unsigned blockLength, const std::vector<unsigned>& frozenBits, int device = 0);
    ~ErrorLocator() override;

    bool decode() override;
    void initialize(size_t blockLength, const std::vector<unsigned>& frozenBits) override;
    void clear();

    int decodeFindFirstError();

    std::vector<float> getOutput();
    void setDesiredOutput(std::vector<float> desired);

    void setAsReferenceDecoder();

    int firstError();
    int correctionCount();

    /// F frames per call, host buffers: llr F x N; desired F x N or null (the defaults: +0 at
    /// information bits, +inf at frozen bits; setDesiredOutput's vector is not used here); outputs u F x N, bits F x N words, first F, count F, each nullable.
    void locateBatch(Mode mode, const float* llr, const float* desired, size_t F, float* u, uint32_t* bits,
                     int32_t* first, uint32_t* count);
    /// Device pointers, asynchronous on `hipStream` (null = default stream).
    void locateBatchDevice(Mode mode, const float* llr, const float* desired, size_t F, float* u, uint32_t* bits,
                           int32_t* first, uint32_t* count, void* hipStream = nullptr);
    int device() const { return mDevice; }
};

} // namespace Decoding
} // namespace PolarCode

#endif
