/* -*- c++ -*- */
// PolarCode::Decoding::FastSscanFloat -- drop-in for the reference's Fast-SSCAN decoder
// (include/polarcode/decoding/fastsscan_float.h:112-132, src/polarcode/decoding/fastsscan_float.cpp):
// SCAN with closed-form rate-0, rate-1, repetition and size-2 subtrees whose passes repeat only
// while the detector check fails, up to the trial limit; on the MI355X (fsscan_kernel.hip through
// pcg_plan_create_fsscan of include/pcg.h).
//
// The reference's members keep their names and meanings: decode() over the signal given by
// setSignal(), decodeAgain() for one more pass, getSoftCodeword() / getSoftInformation() return
// the real per-bit LLRs.  Every value equals the reference's bit for bit for finite LLRs whose
// sums stay finite, with one deliberate difference: every frame starts from reset() state, also
// the message of a TwoBit node that is a right child, which a reused reference instance carries
// over from its previous frame.  setSystematic() has no effect, as in the
// reference.  New: decodeBatch() / decodeBatchSoft() for F frames per call (host buffers) and the
// device-pointer forms.  Construction validates on a host-only plan and needs no GPU.
#ifndef PCA_DEC_FASTSSCAN_H
#define PCA_DEC_FASTSSCAN_H

#include <polarcode/decoding/decoder.h>
#include <vector>

namespace PolarCode {
namespace Decoding {

class FastSscanFloat : public Decoder
{
    unsigned mTrialLimit;
    int mDevice;
    pcg_plan* mPlan = nullptr;
    int mPlanKind = -2;
    unsigned mPasses = 0; // passes the last decode() / decodeAgain() ran; 0: nothing decoded yet

    void ensurePlan();
    void releasePlan();
    bool run(unsigned trials, bool forced);

public:
    FastSscanFloat(size_t blockLength, unsigned trialLimit, const std::vector<unsigned>& frozenBits, int device = 0);
    ~FastSscanFloat() override;

    bool decode() override;
    /// One more pass over the last signal: the passes run so far + 1, without the checks in
    /// between (what the reference's decodeAgain() computes from its kept state).  No node state is
    /// kept here: the signal set by setSignal() is decoded again from the start, so it must still
    /// be the one the last decode() saw.  After a new setSignal() call decode() first (the
    /// reference would run one pass of the new signal on the old frame's messages there).
    bool decodeAgain();
    using Decoder::initialize;
    void initialize(size_t blockLength, unsigned trialLimit, const std::vector<unsigned>& frozenBits);
    void setTrialLimit(unsigned trialLimit);
    void setErrorDetection(ErrorDetection::Detector* pDetector) override;

    /// The trial limit.
    size_t getListSize() override { return mTrialLimit; }
    /// Passes the last decode() / decodeAgain() ran.
    unsigned trials() const { return mPasses; }

    /// F frames per call, host buffers: info F x ceil(K/8), ok F (nullable); `metrics` is ignored.
    bool decodeBatch(const float* llr, size_t F, uint8_t* info, uint8_t* ok = nullptr,
                     float* metrics = nullptr) override;
    /// ... and the soft codewords (F x N floats) and the passes run (F bytes), each nullable.
    bool decodeBatchSoft(const float* llr, size_t F, uint8_t* info, uint8_t* ok, float* soft, uint8_t* trials);
    /// Device pointers, asynchronous on `hipStream` (null = default stream).
    void decodeBatchDevice(const float* llr, size_t F, uint8_t* info, uint8_t* ok = nullptr,
                           float* metrics = nullptr, void* hipStream = nullptr) override;
    void decodeBatchSoftDevice(const float* llr, size_t F, uint8_t* info, uint8_t* ok, float* soft,
                               uint8_t* trials, void* hipStream = nullptr);
    int device() const { return mDevice; }
};

} // namespace Decoding
} // namespace PolarCode

#endif
