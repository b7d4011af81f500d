/* -*- c++ -*- */
// PolarCode::Decoding::DepthFirst -- drop-in for the reference's SC-Flip decoder
// (include/polarcode/decoding/depth_first.h, src/polarcode/decoding/depth_first.cpp): plain
// successive cancellation down to single bits; while the detector check fails, the least reliable
// information-bit decisions are flipped and the frame is decoded again, up to the trial limit; on
// the MI355X (depthfirst_kernel.hip through pcg_plan_create_depthfirst of include/pcg.h).
//
// The reference's members keep their names and meanings: decode() over the signal given by
// setSignal(), setSystematic(), setErrorDetection(); getSoftCodeword() returns the decoded
// codeword's 32-bit words as the reference leaves them (only their sign bits are decisions).
// When the trials run out, the output is the last trial's decode, as in the reference.  Every
// value equals the reference's bit for bit for finite LLRs whose sums stay finite, with one
// deliberate difference: information bits of EQUAL reliability are ordered by their index, where
// the reference's order is whatever std::sort leaves.  setErrorStatistics and
// setNodeRanking, declared but defined nowhere in the reference, are not provided.  New:
// decodeBatch() / decodeBatchBits() for F frames per call (host buffers) and the device-pointer
// forms.  Construction validates on a host-only plan and needs no GPU.
#ifndef PCA_DEC_DEPTHFIRST_H
#define PCA_DEC_DEPTHFIRST_H

#include <polarcode/decoding/decoder.h>
#include <vector>

namespace PolarCode {
namespace Decoding {

class DepthFirst : public Decoder
{
    unsigned mTrialLimit;
    int mDevice;
    pcg_plan* mPlan = nullptr;
    int mPlanKind = -2;
    bool mPlanSystematic = true;
    unsigned mTrials = 0; // trials the last decode() ran; 0: nothing decoded yet

    void ensurePlan();
    void releasePlan();

public:
    DepthFirst(size_t blockLength, size_t trialLimit, const std::vector<unsigned>& frozenBits, int device = 0);
    ~DepthFirst() override;

    bool decode() override;
    using Decoder::initialize;
    void initialize(size_t blockLength, size_t trialLimit, const std::vector<unsigned>& frozenBits);
    void setTrialLimit(size_t trialLimit);
    void setErrorDetection(ErrorDetection::Detector* pDetector) override;

    /// The trial limit.
    size_t getListSize() override { return mTrialLimit; }
    /// Trials the last decode() ran.
    unsigned trials() const { return mTrials; }

    /// F frames per call, host buffers: info F x ceil(K/8), ok F (nullable); `metrics` is ignored.
    bool decodeBatch(const float* llr, size_t F, uint8_t* info, uint8_t* ok = nullptr,
                     float* metrics = nullptr) override;
    /// ... and the decoded words (F x N) and the trials run (F bytes), each nullable.
    bool decodeBatchBits(const float* llr, size_t F, uint8_t* info, uint8_t* ok, uint32_t* bits, uint8_t* trials);
    /// Device pointers, asynchronous on `hipStream` (null = default stream).
    void decodeBatchDevice(const float* llr, size_t F, uint8_t* info, uint8_t* ok = nullptr,
                           float* metrics = nullptr, void* hipStream = nullptr) override;
    void decodeBatchBitsDevice(const float* llr, size_t F, uint8_t* info, uint8_t* ok, uint32_t* bits,
                               uint8_t* trials, void* hipStream = nullptr);
    int device() const { return mDevice; }
};

} // namespace Decoding
} // namespace PolarCode

#endif
