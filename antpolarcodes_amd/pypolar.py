"""Drop-in for the reference's `pypolar` module (python/__init__.py +
python/bindings/*.cc of david13pod/antPolarCodes): PolarDecoder, PolarEncoder,
Detector, Puncturer and frozen_bits with the same names, arguments and errors.

    from antpolarcodes_amd import pypolar
    dec = pypolar.PolarDecoder(1024, 8, pypolar.frozen_bits(1024, 512, 0.0), "gpu")
    dec.setErrorDetection(8)
    bits = dec.decode_vector(llr)            # one frame, as in the reference
    info = dec.decode_batch(llrs)            # (F, N) float32 -> (F, K/8) uint8 on the MI355X

Decoder types "gpu" and "float" run the MI355X kernels (list size < 2 -> Fast-SSC,
else CRC-aided SCL).  ScanDecoder(blockLength, iterationLimit, frozenBitPositions) is the
reference's soft-output SCAN decoder (Decoding::Scan) on the MI355X: real per-bit LLRs from
getSoftCodeword / getExtrinsicChannelInformation and decode_batch(..., return_soft=True); the
decoder type string "scan" of PolarDecoder is not routed to it yet.
FastSscanDecoder(blockLength, trialLimit, frozenBitPositions) is the reference's Fast-SSCAN decoder
(Decoding::FastSscanFloat): the same soft output from closed-form subtrees, passes repeated only
while the detector check fails (decodeAgain() adds one; decode_batch(..., return_trials=True)
reports the passes run).
DepthFirstDecoder(blockLength, trialLimit, frozenBitPositions) is the reference's SC-Flip decoder
(Decoding::DepthFirst): plain successive cancellation, decoded again with the least reliable
information-bit decisions flipped while the detector check fails (decode_batch(...,
return_bits=True, return_trials=True) returns the decoded words and the trials run).
ErrorLocator(blockLength, frozenBitPositions) is the reference's genie-aided SC error locator
(Decoding::ErrorLocator, which the reference's pypolar does not bind: the names are its C++ methods'):
decode_vector, setDesiredOutput, setAsReferenceDecoder, getOutput, firstError, correctionCount,
decodeFindFirstError, and locate_batch(llrs, desired=None, mode="correct") -> (u, bits, first, count).
The native module is mandatory: there is no CPU fallback.
"""
from ._native import _prefer_torch_hip_runtime

_prefer_torch_hip_runtime()  # share PyTorch's HIP runtime (see _native.py)

from ._pypolar import (DepthFirstDecoder, Detector, ErrorLocator, FastSscanDecoder, PolarDecoder, PolarEncoder, Puncturer, ScanDecoder,  # noqa: E402
                       frozen_bits)

__all__ = ["PolarDecoder", "PolarEncoder", "Detector", "Puncturer", "ScanDecoder", "FastSscanDecoder",
           "DepthFirstDecoder", "ErrorLocator", "frozen_bits"]
