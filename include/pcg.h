/*
 * pcg.h -- C ABI of the MI355X polar-code decoder (libpcg.so).
 *
 * This is the drop-in boundary: plain pointers and sizes, no C++ or torch types.
 * The host C++ library (include/polarcode/, mirroring the reference's
 * PolarCode::Decoding::Decoder family) and the Python module (pypolar-compatible)
 * sit on top of it; any other FFI (ctypes, cgo, JNI) can bind it directly.
 *
 * Each entry point replaces a reference interface (paths relative to the
 * reference repository david13pod/antPolarCodes):
 *
 *   pcg_plan_create   <- Decoding::create / makeDecoder + Decoder::initialize,
 *                        src/polarcode/decoding/decoder.cpp:26-87,
 *                        FastSscAvxFloat::initialize fastssc_avx_float.cpp:916-938,
 *                        SclAvxFloat::initialize scl_avx_float.cpp:674-694,
 *                        Decoder::setSystematic decoder.cpp:132,
 *                        Decoder::setErrorDetection decoder.cpp:136
 *   pcg_decode_f32    <- Decoder::decode_vector(const float*, void*) decoder.cpp:154-167,
 *                        batched: F frames per call, device-resident buffers
 *   pcg_decode_f32_host <- the same with host buffers (H2D + decode + D2H)
 *   pcg_decode_f32_soft[_host] <- decode + Decoder::getSoftCodeword (decoder.cpp:147,
 *                        FloatContainer::getSoftBits bitcontainer.cpp:294-297)
 *   pcg_plan_create_adaptive <- makeDecoder(..., 2) = AdaptiveFloat, decoder.cpp:75,
 *                        adaptive_float.cpp:14-45 (SC first, SCL for the failures)
 *   pcg_plan_create_char <- Decoding::create(..., "char") / makeDecoder(..., 0): the 8-bit
 *                        FastSscFipChar (L = 1, fastssc_fip_char.cpp:573-631) and SclFipChar
 *                        (L >= 2, scl_fip_char.cpp:759-856), decoder.cpp:37-38, 62-80
 *   pcg_decode_i8     <- Decoder::decode_vector(const char*, void*) decoder.cpp:169-181,
 *                        batched, device-resident int8 LLRs
 *   pcg_decode_i8_host <- the same with host buffers
 *   pcg_plan_create_adaptive_char <- AdaptiveChar, adaptive_char.cpp:14-45
 *   pcg_plan_create_scan <- new Decoding::Scan(N, iterationLimit, frozen), Scan::initialize
 *                        (src/polarcode/decoding/scan.cpp:17-63) + setSystematic / setErrorDetection
 *   pcg_plan_set_scan_iterations <- Scan::setIterationLimit scan.cpp:26-29
 *   pcg_decode_scan_f32[_host] <- Scan::decode scan.cpp:223-297 (updatellrmap :80-126,
 *                        updatebitmap :128-210), Decoder::getSoftCodeword, and
 *                        Scan::getExtrinsicChannelInformation scan.cpp:299-304, batched
 *   pcg_plan_create_fsscan <- new Decoding::FastSscanFloat(N, trialLimit, frozen)
 *                        (src/polarcode/decoding/fastsscan_float.cpp:269-307, createDecoder :238-265)
 *   pcg_plan_set_fsscan_trials <- the trial limit; forced passes serve decodeAgain :320-325
 *   pcg_decode_fsscan_f32[_host] <- FastSscanFloat::decode :309-339 (RateRNode::decode :116-163,
 *                        RepetitionNode :202-223, TwoBitNode :231-235), batched
 *   pcg_plan_create_depthfirst <- new Decoding::DepthFirst(N, trialLimit, frozen)
 *                        (src/polarcode/decoding/depth_first.cpp:556-597, createDecoder :524-552)
 *   pcg_plan_set_depthfirst_trials <- the trial limit of later decodes
 *   pcg_decode_depthfirst_f32[_host] <- DepthFirst::decode :599-638 (Manager::decode :28-82,
 *                        decodeNext :85-153, RateRNode::decode :277-284), batched
 *   pcg_plan_create_errorlocator <- new Decoding::ErrorLocator(N, frozen)
 *                        (src/polarcode/decoding/errorlocator.cpp:176-210, createDecoder :156-172)
 *   pcg_errorlocator_f32[_host] <- ErrorLocator::decode :214-225 (as the reference decoder or
 *                        with the genie's corrections), decodeFindFirstError :227-232, getOutput,
 *                        firstError, correctionCount, batched
 *   pcg_plan_destroy <- Decoder::~Decoder decoder.cpp:104-114
 *   pcg_last_error    <- the std::exception text the reference throws
 *   pcg_puncturer_*   <- PolarCode::Puncturer (include/polarcode/puncturer.h:33-99,
 *                        src/polarcode/puncturer.cpp:51-89): depuncture / puncture /
 *                        puncturePacked over F frames on the device
 *   pcg_decode_punctured_f32 <- Puncturer::depuncture + Decoder::decode_vector, fused
 *                        into one call (the 5G NR uplink chain)
 *   pcg_encoder_*, pcg_encode <- Encoding::ButterflyFipPacked + Detector::generate
 *                        (src/polarcode/encoding/butterfly_fip_packed.cpp:45-70,
 *                        encoder.cpp:79-90), F frames on the device
 *   pcg_random_info, pcg_bpsk_awgn_f32 <- the simulator's frame source
 *                        (src/simulation/simulator.cpp:850-937, bpsk.cpp:54-80,
 *                        awgn.cpp:38-43), counter-based and reproducible from a seed
 *   pcg_ask_constants, pcg_ask_channel_f32 <- Modulation::Ask, Transmission::Awgn / Rayleigh
 *                        / Scale (ask.cpp:27-101, rayleigh.cpp:76-112), one launch
 *
 *   pcg_plan_set_initial_metric <- the SCL path-metric carry of a reused decoder
 *                        instance (PathList::setFirstPath keeps mMetric[0],
 *                        scl_avx_float.cpp:31, 99-109)
 *
 * Error model: every function returns 0 on success or a negative PCG_E* code;
 * nothing throws across the ABI.  pcg_last_error() (thread-local) describes the
 * most recent failure on the calling thread.
 *
 * Threading and streams: a plan is like the reference's stateful Decoder objects (one per
 * worker thread, simulator.cpp:703-764): its scratch, work queue, staging and adaptive
 * frame-map buffers are reused by every decode call, so a plan must be used from one host
 * thread at a time.  Decodes of one plan may be issued on different streams: each decode
 * waits (hipStreamWaitEvent) for the plan's previous decode, whichever stream ran it, so
 * they never overlap; the SCL work-queue counter is zeroed on the launch stream before
 * every launch; pcg_plan_destroy waits for the plan's last decode before freeing.  Plans
 * are independent of each other: one plan per stream / per GPU runs concurrently.
 */
#ifndef PCG_H
#define PCG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PCG_OK 0
#define PCG_E_ARG (-1)         /* bad argument (sizes, null pointers, N not a power of 2) */
#define PCG_E_FROZEN (-2)      /* frozen pattern the reference rejects with std::invalid_argument
                                  (fastssc_avx_float.cpp:821-825, 839-843) */
#define PCG_E_HIP (-3)         /* HIP runtime error (allocation, launch, copy) */
#define PCG_E_UNSUPPORTED (-4) /* valid for the reference, not (yet) for this build */
#define PCG_E_NODEVICE (-5)    /* no GPU / HIP runtime unavailable */

/* Error-detection kind used to choose the SCL output path and to fill `ok`
 * (ErrorDetection::create(size, "crc"), errordetector.cpp:23-67). */
#define PCG_CRC_NONE 0  /* Dummy: check() always true (dummy.cpp:27)                 */
#define PCG_CRC8 8      /* CRC-8, poly 0x07 (crc8.cpp)                              */
#define PCG_CRC11 11    /* 3GPP TS 38.212 CRC-11 over the bit stream, parity in the
                           last 11 bits -- NOT in the reference     */
#define PCG_CRC16 16    /* CRC-16/CCITT-FALSE, big-endian trailer (crc16.cpp)       */
#define PCG_CRC32C 32   /* CRC-32C over little-endian words (crc32.cpp)             */

typedef struct pcg_plan pcg_plan;

typedef struct pcg_plan_desc {
    uint32_t block_length;  /* N */
    uint32_t info_length;   /* K = N - |frozen| */
    uint32_t list_size;     /* L (1 = Fast-SSC) */
    uint32_t node_count;    /* decoder tree nodes */
    uint32_t op_count;      /* flattened schedule length */
    uint32_t lds_bytes;     /* LDS per codeword */
    uint64_t scratch_bytes; /* global scratch per codeword */
    int32_t crc_kind;
    int32_t systematic;
    uint32_t lanes_per_codeword; /* SCL: lanes of a wave per codeword (list size rounded up, or
                                    wider); Fast-SSC scq kernel: its Q; 0 for the other kernels */
    uint32_t dev_overrides;      /* PCG_DEV_* bits: developer environment switches
                                    that changed this plan's kernel or layout; 0 in production */
    uint32_t recomputed_stages;  /* lane-serial SCL: top LLR stages recomputed from the channel
                                    where read instead of stored (1: the root's children, 2:
                                    also its grandchildren); 0 for the other kernels */
    uint32_t specialized;        /* 1: decodes run the plan-specialised kernel (pcg_plan_specialize;
                                    an adaptive plan: both of its stages) */
} pcg_plan_desc;

#define PCG_DEV_SCL_LP 0x1   /* PCG_SCL_LP / PCG_ADAPT_LP (only when the caller passed 0) */
#define PCG_DEV_SCL_FUSE 0x2 /* PCG_SCL_FUSE */
#define PCG_DEV_SCQ 0x4      /* PCG_SCQ_Q / PCG_SCQ_VIRT */
#define PCG_DEV_LAYOUT 0x8   /* PCG_SC_KERNEL, PCG_*_LDS_KB, PCG_*_SL, PCG_*_WPC, PCG_SCL_VIRT, ... */
#define PCG_DEV_OPPROF 0x10  /* PCG_OPPROF */
#define PCG_DEV_FLAGS 0x20   /* PCG_FLAGS */
#define PCG_DEV_BUILD 0x40   /* a development build of the list kernel (compile-time knobs != defaults) */

/* Build a decoding plan: classify the decoder tree exactly as the reference
 * (Fast-SSC for L == 1, SCL for L >= 2), flatten it to a device schedule and
 * upload it to `device`.  `frozen` must be strictly ascending indices < N.
 * crc_kind: PCG_CRC_NONE/8/11/16/32.  L <= 32. */
int pcg_plan_create(pcg_plan** plan,
                    uint32_t N,
                    uint32_t L,
                    const uint32_t* frozen,
                    uint32_t n_frozen,
                    int systematic,
                    int crc_kind,
                    int device);

/* An adaptive plan (makeDecoder's "mixed" = AdaptiveFloat, decoder.cpp:40-41, 75;
 * adaptive_float.cpp:33-45): pcg_decode_f32 first decodes every frame with Fast-SSC, then
 * re-decodes the frames whose detector check failed with CRC-aided SCL (list size L); a
 * re-decoded frame reports the SCL output and ok flag.  metrics: the SCL path metrics of
 * re-decoded frames, 0 for frames Fast-SSC settled.  Asynchronous (the failed-frame list
 * stays on the device).  L < 2 creates a plain Fast-SSC plan.  Fails like both decoders'
 * constructors (PCG_E_FROZEN for frozen patterns Fast-SSC rejects). */
int pcg_plan_create_adaptive(pcg_plan** plan,
                             uint32_t N,
                             uint32_t L,
                             const uint32_t* frozen,
                             uint32_t n_frozen,
                             int systematic,
                             int crc_kind,
                             int device);

/* Decode F frames.  llr: device pointer, F x N float32 (natural order, LLR > 0
 * <=> bit 0).  info: device pointer, F x ceil(K/8) bytes (MSB-first info bits,
 * exactly Decoder::getDecodedInformationBits).  ok: device pointer to F bytes
 * (Decoder::decode's return value) or NULL.  metrics: device pointer, F x L
 * floats of the final ordered SCL path metrics (unused path slots = 0), or NULL
 * (ignored for L == 1).  stream: hipStream_t or NULL for the null stream.
 * Asynchronous with respect to the host. */
int pcg_decode_f32(pcg_plan* plan,
                   const float* llr,
                   uint64_t F,
                   uint8_t* info,
                   uint8_t* ok,
                   float* metrics,
                   void* stream);

/* Same contract with HOST pointers; synchronous.  Streams the batch through
 * device buffers in chunks. */
int pcg_decode_f32_host(pcg_plan* plan,
                        const float* llr,
                        uint64_t F,
                        uint8_t* info,
                        uint8_t* ok,
                        float* metrics);

/* Fast-SSC float plans (L == 1): decode as pcg_decode_f32 and also write each frame's soft
 * codeword -- the reference's root FloatContainer word for word (Decoder::getSoftCodeword,
 * decoder.cpp:147; the leaf decoders' float outputs combined by the full 32-bit XOR of
 * RateRNode, fastssc_avx_float.cpp:148-792).  soft: device F x N floats.  Runs the
 * one-codeword-per-wave kernel (slower than pcg_decode_f32).  PCG_E_UNSUPPORTED for list,
 * 8-bit and adaptive plans and for N whose state exceeds a CU's LDS (N > 16384). */
int pcg_decode_f32_soft(pcg_plan* plan,
                        const float* llr,
                        uint64_t F,
                        uint8_t* info,
                        uint8_t* ok,
                        float* soft,
                        void* stream);

/* Same with HOST pointers; synchronous. */
int pcg_decode_f32_soft_host(pcg_plan* plan,
                             const float* llr,
                             uint64_t F,
                             uint8_t* info,
                             uint8_t* ok,
                             float* soft);

/* An 8-bit fixed-point plan: the reference's "char" decoders (FastSscFipChar for L == 1,
 * SclFipChar for L >= 2; L <= 32), classified and computed exactly as they are
 * (saturating int8 LLRs, integer path metrics).  Decode int8 frames with pcg_decode_i8, or
 * float frames with pcg_decode_f32 (quantised in the kernel as CharContainer::insertLlr
 * does, bitcontainer.cpp:449-516).  `metrics` of such plans are the integer SCL path
 * metrics as floats (exact).  Non-systematic decoding follows the reference's intent
 * (re-encode, then extract); for N < 256 the reference's own output is undefined there
 * (DESIGN.md Q9). */
int pcg_plan_create_char(pcg_plan** plan,
                         uint32_t N,
                         uint32_t L,
                         const uint32_t* frozen,
                         uint32_t n_frozen,
                         int systematic,
                         int crc_kind,
                         int device);

/* The 8-bit adaptive decoder AdaptiveChar (adaptive_char.cpp:14-45; pcsim's 8-bit list
 * decoding, simulator.cpp:722-727): FastSscFipChar for every frame, SclFipChar for the
 * frames whose check failed, as pcg_plan_create_adaptive does for the float decoders. */
int pcg_plan_create_adaptive_char(pcg_plan** plan,
                                  uint32_t N,
                                  uint32_t L,
                                  const uint32_t* frozen,
                                  uint32_t n_frozen,
                                  int systematic,
                                  int crc_kind,
                                  int device);

/* Decode F frames of int8 LLRs (device pointer, F x N bytes) with an 8-bit plan; outputs
 * as pcg_decode_f32.  PCG_E_ARG for a float plan.  Asynchronous. */
int pcg_decode_i8(pcg_plan* plan,
                  const int8_t* llr,
                  uint64_t F,
                  uint8_t* info,
                  uint8_t* ok,
                  float* metrics,
                  void* stream);

/* Same contract with HOST pointers; synchronous. */
int pcg_decode_i8_host(pcg_plan* plan,
                       const int8_t* llr,
                       uint64_t F,
                       uint8_t* info,
                       uint8_t* ok,
                       float* metrics);

/* ---- SCAN: the soft-output cancellation decoder (Decoding::Scan, scan.cpp) ----------------
 * A SCAN plan runs `iterations` (0 .. 255) passes of the reference's message schedule over each
 * frame and returns real per-bit LLRs: the soft codeword (channel + extrinsic for systematic
 * plans, the per-leaf sums for non-systematic ones) and the extrinsic channel information.
 * Every frame starts from zeroed state: nothing carries between frames or calls.  All outputs
 * equal the reference's bit for bit, signed zeros and infinities included (a non-systematic
 * decode with 0 iterations returns +0.0, a freshly constructed reference decoder's output).
 * Contract: finite LLRs whose sums stay finite -- outside that the reference itself produces
 * NaN, and the pruning of all-frozen subtrees here need not reproduce it.
 * N: a power of two, 8 <= N <= 4096 (PCG_E_UNSUPPORTED above); any strictly ascending frozen
 * set (PCG_E_FROZEN never applies).  pcg_plan_describe reports list_size = iterations (as
 * Scan::getListSize does), lds_bytes of a wave and scratch_bytes per codeword;
 * pcg_plan_kernel_name is "scan_kernel".  There is no specialised kernel, no 8-bit form and no
 * punctured decode: pcg_plan_specialize[_async], pcg_decode_i8[_host] and
 * pcg_decode_punctured_f32 return PCG_E_UNSUPPORTED.  pcg_decode_f32[_host] on a SCAN plan
 * writes info and ok (metrics is ignored); pcg_decode_f32_soft[_host] also the soft codeword. */
int pcg_plan_create_scan(pcg_plan** plan,
                         uint32_t N,
                         uint32_t iterations,
                         const uint32_t* frozen,
                         uint32_t n_frozen,
                         int systematic,
                         int crc_kind,
                         int device);

/* Scan::setIterationLimit: the iteration count of later decodes (0 .. 255). */
int pcg_plan_set_scan_iterations(pcg_plan* plan, uint32_t iterations);

/* Decode F frames with a SCAN plan (PCG_E_ARG for any other plan).  Device pointers,
 * asynchronous, stream-ordered like pcg_decode_f32.  info: F x ceil(K/8) bytes, the sign bits
 * of the soft codeword at the information positions, MSB-first.  ok (F bytes), soft and
 * extrinsic (F x N floats each, natural order) may be NULL: an output not asked for costs no
 * stores. */
int pcg_decode_scan_f32(pcg_plan* plan,
                        const float* llr,
                        uint64_t F,
                        uint8_t* info,
                        uint8_t* ok,
                        float* soft,
                        float* extrinsic,
                        void* stream);

/* Same with HOST pointers; synchronous.  Streams the batch through device buffers in chunks. */
int pcg_decode_scan_f32_host(pcg_plan* plan,
                             const float* llr,
                             uint64_t F,
                             uint8_t* info,
                             uint8_t* ok,
                             float* soft,
                             float* extrinsic);

/* ---- Fast-SSCAN: SCAN with closed-form subtrees and detector-terminated passes ------------
 * (Decoding::FastSscanFloat, fastsscan_float.cpp.)  The same factor graph as SCAN in natural
 * index order; rate-0, rate-1, repetition and size-2 subtrees are closed forms, and a pass is
 * repeated only while the frame's detector check fails, up to trial_limit (1 .. 255; 0 is
 * PCG_E_ARG: the reference would return stale output).  Outputs equal the reference's bit for
 * bit: the soft codeword (channel LLR + root message), the info bytes (its sign bits at the
 * information positions) and ok; `trials` is the number of passes each frame ran.  With the
 * dummy detector (crc_kind 0) every frame stops after pass 1.  Frames are independent: every
 * frame starts from reset() state -- also the message of a right-child TwoBit node, which a
 * reused reference instance carries over from its previous frame.
 * `systematic` is recorded for pcg_plan_describe and otherwise ignored, as in the reference.
 * Contract: finite LLRs whose sums stay finite.  N: a power of two, 8 <= N <= 4096
 * (PCG_E_UNSUPPORTED above); any strictly ascending frozen set.  pcg_plan_describe reports
 * list_size = trial_limit, lds_bytes of a wave and scratch_bytes per codeword;
 * pcg_plan_kernel_name is "fsscan_kernel".  pcg_decode_f32[_host] and pcg_decode_f32_soft[_host]
 * work as on a SCAN plan; pcg_plan_specialize[_async], pcg_decode_i8[_host] and
 * pcg_decode_punctured_f32 return PCG_E_UNSUPPORTED, pcg_decode_scan_f32[_host] PCG_E_ARG. */
int pcg_plan_create_fsscan(pcg_plan** plan,
                           uint32_t N,
                           uint32_t trial_limit,
                           const uint32_t* frozen,
                           uint32_t n_frozen,
                           int systematic,
                           int crc_kind,
                           int device);

/* The trial limit (1 .. 255) of later decodes.  forced != 0: run exactly trial_limit passes and
 * ignore the check in between; ok is the check after the last pass (FastSscanFloat::decodeAgain
 * after t passes = t + 1 forced passes; fixed-pass soft output with the dummy detector). */
int pcg_plan_set_fsscan_trials(pcg_plan* plan, uint32_t trial_limit, int forced);

/* Decode F frames with a Fast-SSCAN plan (PCG_E_ARG for any other plan).  Device pointers,
 * asynchronous, stream-ordered like pcg_decode_f32.  info: F x ceil(K/8) bytes.  ok (F bytes),
 * soft (F x N floats, natural order) and trials (F bytes) may be NULL: an output not asked for
 * costs no stores. */
int pcg_decode_fsscan_f32(pcg_plan* plan,
                          const float* llr,
                          uint64_t F,
                          uint8_t* info,
                          uint8_t* ok,
                          float* soft,
                          uint8_t* trials,
                          void* stream);

/* Same with HOST pointers; synchronous.  Streams the batch through device buffers in chunks. */
int pcg_decode_fsscan_f32_host(pcg_plan* plan,
                               const float* llr,
                               uint64_t F,
                               uint8_t* info,
                               uint8_t* ok,
                               float* soft,
                               uint8_t* trials);

/* ---- SC-Flip: successive cancellation with detector-driven bit flips ----------------------
 * (Decoding::DepthFirst, depth_first.cpp.)  A frame is decoded with plain successive cancellation
 * down to single bits; while its detector check fails, the reference's search configures the
 * least reliable information-bit decisions (|LLR| at the leaf) to be flipped and the frame is
 * decoded again, up to trial_limit full decodes (1 .. 255).  When the trials run out the output
 * is the LAST trial's decode, as in the reference.  Outputs equal the reference's bit for bit:
 * the info bytes (sign bits at the information positions; a non-systematic plan re-encodes
 * first), ok, and `bits`, the F x N 32-bit words of the decoded codeword that getSoftCodeword
 * returns (an information leaf's LLR, negated where flipped, +inf at a frozen leaf, XOR-combined
 * upwards: only the sign bits are decisions); `trials` is the number of decodes each frame ran.
 * With the dummy detector (crc_kind 0) every frame stops after trial 1.  One deviation: leaves
 * of EQUAL reliability are ordered by leaf index here (a stable sort), where the reference's
 * order is whatever std::sort leaves; frames whose search meets no tie are
 * identical.  Contract: finite LLRs whose sums stay finite.  N: a power of two, 8 <= N <= 4096
 * (PCG_E_UNSUPPORTED above); any strictly ascending frozen set with K >= max(trial_limit, 2)
 * information bits (PCG_E_ARG below: the reference reads past its reliability list).
 * pcg_plan_describe reports list_size = trial_limit, lds_bytes of a wave and scratch_bytes per
 * codeword; pcg_plan_kernel_name is "depthfirst_kernel".  pcg_decode_f32[_host] work;
 * pcg_plan_specialize[_async], pcg_decode_f32_soft[_host], pcg_decode_i8[_host] and
 * pcg_decode_punctured_f32 return PCG_E_UNSUPPORTED, the SCAN and Fast-SSCAN entry points
 * PCG_E_ARG. */
int pcg_plan_create_depthfirst(pcg_plan** plan,
                               uint32_t N,
                               uint32_t trial_limit,
                               const uint32_t* frozen,
                               uint32_t n_frozen,
                               int systematic,
                               int crc_kind,
                               int device);

/* The trial limit (1 .. 255, at most K) of later decodes. */
int pcg_plan_set_depthfirst_trials(pcg_plan* plan, uint32_t trial_limit);

/* Decode F frames with an SC-Flip plan (PCG_E_ARG for any other plan).  Device pointers,
 * asynchronous, stream-ordered like pcg_decode_f32.  info: F x ceil(K/8) bytes.  ok (F bytes),
 * bits (F x N words, natural order) and trials (F bytes) may be NULL: an output not asked for
 * costs no stores. */
int pcg_decode_depthfirst_f32(pcg_plan* plan,
                              const float* llr,
                              uint64_t F,
                              uint8_t* info,
                              uint8_t* ok,
                              uint32_t* bits,
                              uint8_t* trials,
                              void* stream);

/* Same with HOST pointers; synchronous.  Streams the batch through device buffers in chunks. */
int pcg_decode_depthfirst_f32_host(pcg_plan* plan,
                                   const float* llr,
                                   uint64_t F,
                                   uint8_t* info,
                                   uint8_t* ok,
                                   uint32_t* bits,
                                   uint8_t* trials);

/* ---- The genie-aided SC error locator ("bad bit finder") --------------------------------------
 * (Decoding::ErrorLocator, errorlocator.cpp.)  Plain successive cancellation down to single bits
 * in which a leaf outputs either its LLR or a DESIRED value, as a whole 32-bit float.  A frozen
 * leaf always outputs its desired value.  `desired` is F x N floats, all N positions honoured
 * (setDesiredOutput); NULL means the reference's defaults, +0.0f at information bits and +inf at
 * frozen bits.  Only the SIGN BITS of the desired values at information bits are compared (a
 * signed zero counts).  The mode is fixed per call:
 *   PCG_EL_REFERENCE  setAsReferenceDecoder() + decode(): no comparison; first = -1, count = 0.
 *   PCG_EL_CORRECT    decode(): every information bit whose sign differs from its desired value's
 *                     outputs the desired value instead.  first = index (among all N bits) of the
 *                     first bit replaced or -1 (firstError()), count = bits replaced
 *                     (correctionCount()).  The reference repeats the root decode once per
 *                     replacement; SC is causal, so its final state equals ONE decode that
 *                     compares and replaces each leaf when it is reached, which is what runs here.
 *   PCG_EL_FIRST      decodeFindFirstError(): compare, never replace.  first = index of the first
 *                     mismatch or -1; count = 0.
 * Outputs, each may be NULL and one not asked for costs no stores: u (F x N floats, getOutput():
 * an LLR, a desired value, or +inf), bits (F x N 32-bit words, getSoftCodeword: the leaf words
 * XOR-combined upwards), first (F x int32), count (F x uint32).  Every value equals the
 * reference's bit for bit.  Contract: finite LLRs whose sums stay finite.  N: a power of two,
 * 8 <= N <= 4096 (PCG_E_UNSUPPORTED above); any strictly ascending frozen set that leaves at least
 * one information bit.  The decoder produces no information bytes and has no detector.
 * pcg_plan_describe reports lds_bytes of a wave, node_count / op_count as the SC-Flip plan of the
 * same code, and scratch_bytes per codeword = 4 * 4 N: the node inputs per level (2 N words), the
 * decoded words (N) and the desired / leaf values (N).  pcg_plan_kernel_name is
 * "errorlocator_kernel".  On such a plan pcg_decode_f32[_host], pcg_decode_f32_soft[_host],
 * pcg_decode_i8[_host], pcg_decode_punctured_f32 and pcg_plan_specialize[_async] return
 * PCG_E_UNSUPPORTED, the SCAN, Fast-SSCAN and SC-Flip entry points PCG_E_ARG. */
#define PCG_EL_REFERENCE 0
#define PCG_EL_CORRECT 1
#define PCG_EL_FIRST 2

int pcg_plan_create_errorlocator(pcg_plan** plan, uint32_t N, const uint32_t* frozen, uint32_t n_frozen, int device);

/* Run F frames through an error-locator plan.  Device pointers, asynchronous, stream-ordered like
 * pcg_decode_f32.  PCG_E_ARG for an unknown mode, a NULL llr or any other plan. */
int pcg_errorlocator_f32(pcg_plan* plan,
                         int mode,
                         const float* llr,
                         const float* desired,
                         uint64_t F,
                         float* u,
                         uint32_t* bits,
                         int32_t* first,
                         uint32_t* count,
                         void* stream);

/* Same with HOST pointers; synchronous.  Streams the batch through device buffers in chunks. */
int pcg_errorlocator_f32_host(pcg_plan* plan,
                              int mode,
                              const float* llr,
                              const float* desired,
                              uint64_t F,
                              float* u,
                              uint32_t* bits,
                              int32_t* first,
                              uint32_t* count);

int pcg_plan_describe(const pcg_plan* plan, pcg_plan_desc* desc);

/* Name of the kernel a decode on this plan launches (e.g. "sclls_kernel<8>",
 * "scs_kernel"), as it appears in rocprofv3 kernel traces; "" for NULL. */
const char* pcg_plan_kernel_name(const pcg_plan* plan);

/* Compile (hiprtc, at run time) and load a kernel specialised to this plan's code: the
 * LDS-resident Fast-SSC kernel with the plan's decoder tree as a compile-time schedule, the
 * lane-serial list kernel with the plan's layout and constants as literals, and for 8-bit
 * plans the lane-serial FastSscFipChar / SclFipChar kernels with their constants and layout as
 * literals (sccs_rtc_kernel / scl_char_rtc_kernel) -- the same device code and arithmetic as
 * the interpreter kernels, so the same outputs bit for bit.  An adaptive plan specialises both
 * of its stages.  This
 * replaces the reference's per-code decoder object tree (FastSscAvx::createDecoder,
 * fastssc_avx_float.cpp:797-896; SclAvx::createDecoder, scl_avx_float.cpp:624-651) with
 * per-code machine code.  Code objects are cached per process, in the library's shipped
 * cache (<dir of libpcg.so>/rtc, filled at build time for the catalogue of
 * antpolarcodes_amd/rtc_codes.py: the benchmark configurations and a validation catalogue) and
 * on disk (PCG_RTC_CACHE); a code in none of them takes tens of seconds of hiprtc once.
 * Plans do this by themselves: with a cached code object from their first decode, otherwise
 * in a background thread from their first decode of >= 8192 frames, switching once it is
 * ready (PCG_RTC=0 never, PCG_RTC=1 at the first decode, waiting).  PCG_E_UNSUPPORTED for
 * the 8-bit Fast-SSC plans that run the one-codeword-per-wave kernel and with PCG_OPPROF; on
 * a host-only plan it only compiles.  On failure (no hiprtc, a device of another
 * architecture) the plan keeps decoding with the interpreter kernel.  Plans of one code
 * share one compile; pcg_plan_destroy never waits for it, process exit does (with a notice
 * on stderr; PCG_RTC_EXIT_WAIT=<s> bounds that wait).  The first compile a process starts is
 * preceded by a short warm-up compile (~1-2 s, loading hiprtc's compiler) on the calling
 * thread, so the first pcg_plan_specialize_async -- or the first decode of >= 8192 frames
 * that starts a compile -- can block for that long. */
int pcg_plan_specialize(pcg_plan* plan);

/* Start pcg_plan_specialize without waiting: the plan switches at a later decode (or
 * pcg_plan_specialize) once the code object is ready.  Returns without waiting for the
 * compile (only the process's first compile is preceded by the warm-up above). */
int pcg_plan_specialize_async(pcg_plan* plan);

/* SCL plans: the metric path 0 starts every frame of later decode calls with.  0 (the
 * default) is a freshly constructed reference decoder; passing the previous frame's final
 * metrics[0] reproduces a reference decoder instance reused frame after frame (its
 * PathList never resets mMetric, scl_avx_float.cpp:31, 99-109).  For the
 * 8-bit plans the value is converted to the integer metric.  Ignored by Fast-SSC. */
int pcg_plan_set_initial_metric(pcg_plan* plan, float metric0);

void pcg_plan_destroy(pcg_plan* plan);

const char* pcg_last_error(void);

/* Number of HIP devices visible (0 without a GPU); never fails. */
int pcg_device_count(void);

/* ---- rate matching: Puncturer --------------------------------------------------------
 * Puncturer(blockLength = E, frozenBitPositions): parent length N = next power of two
 * >= E; the first N - E entries of `frozen` (as given; frozen_bits returns them
 * ascending) are punctured; PCG_E_ARG with the reference's std::out_of_range text
 * ("Number of required puncturing positions exceeds frozen bit positions!") when the
 * frozen set is too small.  device < 0: host-only (positions, no device tables). */
typedef struct pcg_puncturer pcg_puncturer;

int pcg_puncturer_create(pcg_puncturer** punc,
                         uint32_t E,
                         const uint32_t* frozen,
                         uint32_t n_frozen,
                         int device);

/* E, N and (if `positions` is not NULL) the E kept parent positions, ascending
 * (Puncturer::blockLength / parentBlockLength / blockOutputPositions). */
int pcg_puncturer_describe(const pcg_puncturer* punc, uint32_t* E, uint32_t* N, uint32_t* positions);

/* Device buffers, asynchronous on `stream`:
 *   depuncture  in F x E floats -> out F x N floats, punctured positions = +0.0f
 *   puncture    in F x N floats -> out F x E floats
 *   puncture_packed  in F x N/8 MSB-first bytes -> out F x E/8 (E, N multiples of 8) */
int pcg_depuncture_f32(const pcg_puncturer* punc, const float* in, uint64_t F, float* out, void* stream);
int pcg_puncture_f32(const pcg_puncturer* punc, const float* in, uint64_t F, float* out, void* stream);
int pcg_puncture_packed(const pcg_puncturer* punc, const uint8_t* in, uint64_t F, uint8_t* out, void* stream);

void pcg_puncturer_destroy(pcg_puncturer* punc);

/* Decode F punctured frames: llr is F x E (device), depunctured on the device and decoded
 * with `plan` (whose N must equal the puncturer's parent length).  Outputs as
 * pcg_decode_f32.  Float list plans depuncture inside the decode kernel (each wave its
 * codeword group, into its scratch: one launch, no staging buffer); the other plans
 * depuncture into a plan staging buffer first (reused across calls, ordered after the
 * plan's previous decode).  Stream-ordered. */
int pcg_decode_punctured_f32(pcg_plan* plan,
                             const pcg_puncturer* punc,
                             const float* llr,
                             uint64_t F,
                             uint8_t* info,
                             uint8_t* ok,
                             float* metrics,
                             void* stream);

/* ---- frame source: encoder, random information, BPSK-AWGN channel ---------------------- */
typedef struct pcg_encoder pcg_encoder;

/* ButterflyFipPacked(N, frozen) + setSystematic + setErrorDetection(crc_kind). */
int pcg_encoder_create(pcg_encoder** enc,
                       uint32_t N,
                       const uint32_t* frozen,
                       uint32_t n_frozen,
                       int systematic,
                       int crc_kind,
                       int device);

/* info: device F x ceil(K/8) bytes; the detector's check bits are written into it in
 * place (as encode_vector does to its caller's buffer).  code: device F x N/8 bytes,
 * MSB-first (Encoder::getEncodedData). */
int pcg_encode(pcg_encoder* enc, uint8_t* info, uint64_t F, uint8_t* code, void* stream);

void pcg_encoder_destroy(pcg_encoder* enc);

/* Uniform random information bytes (device F x ceil(K/8)), bits past K cleared:
 * Philox4x32-10 keyed by `seed`, counter = (frame, byte block). */
int pcg_random_info(uint8_t* info, uint64_t F, uint32_t K, uint64_t seed, void* stream);

/* BPSK (bit 0 -> +1) + AWGN of standard deviation sigma + LLR = 2 y / sigma^2 over n
 * packed code bits per frame (device code F x n/8 -> llr F x n floats, n % 8 == 0).
 * sigma <= 0: noiseless, llr = +-1.  Noise from Philox4x32-10 keyed by `seed`. */
int pcg_bpsk_awgn_f32(const uint8_t* code, uint64_t F, uint32_t n, float sigma, uint64_t seed, float* llr,
                      void* stream);

/* ---- ASK modulation, AWGN or Rayleigh fading, soft demodulation, scaling ----------------
 * (Modulation::Ask, ask.cpp:27-101; Transmission::Awgn / Rayleigh / Scale.)  One launch from
 * packed code bits (device F x n/8 bytes, MSB-first, n % 8 == 0) to the floats a decoder
 * reads (device F x n).  A frame has S = ceil(n / bits_per_symbol) symbols; code bits past n
 * count as 0 and their outputs are not written.  Per symbol:
 *   x = level * power_normalizer            level: m = 1, s = 0; per bit m *= (bit ? -1 : +1),
 *                                           s = 2 s + m
 *   y = x + sigma g                         PCG_FADING_NONE
 *   y = x sqrtf(g1 g1 + g2 g2) + sigma g    PCG_FADING_RAYLEIGH: the fading is not normalised
 *                                           (E[h^2] = 2) and not equalised, as in the reference
 *   a = y * normal_magnitude; per bit k: out = gain * a, a = |a| - 2^(b-1-k)
 * sigma <= 0: no additive noise (Rayleigh still fades).  g, g1, g2 are standard normals from
 * Philox4x32-10 keyed by `seed`, a pure function of (seed, frame, symbol index); with
 * bits_per_symbol = 1 and PCG_FADING_NONE y equals pcg_bpsk_awgn_f32's noisy symbol bit for
 * bit (that call returns y * 2 / sigma^2).  symbols: device F x S floats receiving y, or NULL.
 * PCG_E_ARG for bits_per_symbol outside 1 .. 16, an unknown fading, n % 8 != 0 or a NULL code /
 * out; a no-op for F == 0.  Asynchronous. */
#define PCG_FADING_NONE 0 /* AWGN */
#define PCG_FADING_RAYLEIGH 1

/* Ask::setBitsPerSymbol's mNormalMagnitude and mPowerNormalizer (host only, no device). */
int pcg_ask_constants(uint32_t bits_per_symbol, float* normal_magnitude, float* power_normalizer);

int pcg_ask_channel_f32(const uint8_t* code, uint64_t F, uint32_t n, uint32_t bits_per_symbol, int fading,
                        float sigma, float gain, uint64_t seed, float* out, float* symbols /* may be NULL */,
                        void* stream);

#ifdef __cplusplus
}
#endif

#endif /* PCG_H */
