/* -*- c++ -*- */
// PolarCode::Decoding::Scan -- drop-in for the reference's SCAN decoder
// (include/polarcode/decoding/scan.h:26-58, src/polarcode/decoding/scan.cpp): Soft-output
// CANcellation after "Low-Complexity Soft-Output Decoding of Polar Codes" by Ubaid U. Fayyaz and
// John R. Barry, on the MI355X (scan_kernel.hip through pcg_plan_create_scan of include/pcg.h).
//
// The reference's members keep their names and meanings: decode() over the signal given by
// setSignal(), getSoftCodeword() / getSoftInformation() return the real per-bit LLRs,
// getExtrinsicChannelInformation() the extrinsic part, getListSize() the iteration limit.
// Every value equals the reference's bit for bit for finite LLRs whose sums stay finite.
// New: decodeBatch() / decodeBatchSoft() for F frames per call (host buffers) and the
// device-pointer forms.  Construction validates on a host-only plan and needs no GPU.
//
// Decoding::create(..., "scan") and makeDecoder(..., 3) still refuse (decoder.h); construct
// this class directly.
#ifndef PCA_DEC_SCAN_H
#define PCA_DEC_SCAN_H

#include <polarcode/decoding/decoder.h>
#include <vector>

namespace PolarCode {
namespace Decoding {

class Scan : public Decoder
{
    unsigned mIterationLimit;
    int mDevice;
    pcg_plan* mPlan = nullptr;
    int mPlanKind = -2;
    bool mPlanSys = true;
    std::vector<float> mExtrinsic;

    void ensurePlan();
    void releasePlan();

public:
    Scan(size_t blockLength, unsigned iterationLimit, const std::vector<unsigned>& frozenBits, int device = 0);
    ~Scan() override;

    bool decode() override;
    using Decoder::initialize;
    void initialize(size_t blockLength, unsigned iterationLimit, const std::vector<unsigned>& frozenBits);
    void setIterationLimit(unsigned iterationLimit);
    void setErrorDetection(ErrorDetection::Detector* pDetector) override;

    /// The extrinsic channel LLRs of the last decode() (N floats, natural order).
    void getExtrinsicChannelInformation(float*);

    /// The iteration limit, as the reference's Scan::getListSize.
    size_t getListSize() override { return mIterationLimit; }

    /// F frames per call, host buffers: info F x ceil(K/8), ok F (nullable); `metrics` is ignored.
    bool decodeBatch(const float* llr, size_t F, uint8_t* info, uint8_t* ok = nullptr,
                     float* metrics = nullptr) override;
    /// ... and the soft codewords / extrinsic channel information, F x N floats each (nullable).
    bool decodeBatchSoft(const float* llr, size_t F, uint8_t* info, uint8_t* ok, float* soft, float* extrinsic);
    /// Device pointers, asynchronous on `hipStream` (null = default stream).
    void decodeBatchDevice(const float* llr, size_t F, uint8_t* info, uint8_t* ok = nullptr,
                           float* metrics = nullptr, void* hipStream = nullptr) override;
    void decodeBatchSoftDevice(const float* llr, size_t F, uint8_t* info, uint8_t* ok, float* soft,
                               float* extrinsic, void* hipStream = nullptr);
    int device() const { return mDevice; }
};

} // namespace Decoding
} // namespace PolarCode

#endif
