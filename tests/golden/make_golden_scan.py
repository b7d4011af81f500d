#!/usr/bin/env python3
"""Generate tests/golden/scan_fixtures.npz from the REFERENCE's SCAN decoder.

Runs only where oracle/_ref/libpolarref.so was built from /root/reference's sources
(`make -C oracle ref`).  A small C++ shim of our own (below) is compiled into a temporary
directory against the reference's headers and that library; it constructs
`new Decoding::Scan(N, iterations, frozen)` and records decode_vector, getSoftCodeword and
getExtrinsicChannelInformation.  Nothing compiled is kept.  Data only: inputs and the
reference's outputs.  tests/test_scan_restatement.py pins tests/scan_numpy.py to these fixtures;
tests/test_gpu_scan.py checks the HIP kernel against both.

    python tests/golden/make_golden_scan.py
"""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

from helpers import LLR_KINDS, llr_kinds  # noqa: E402

from antpolarcodes_amd.construction import frozen_bits  # noqa: E402

REF = "/root/reference"
REF_SO_DIR = os.path.join(ROOT, "oracle", "_ref")

SHIM = r"""
#include <polarcode/decoding/scan.h>
#include <polarcode/errordetection/errordetector.h>
#include <chrono>
#include <vector>
using namespace PolarCode;
// F frames through one Scan decoder; returns the seconds the decode_vector calls took
extern "C" double scan_ref(unsigned N, unsigned it, const unsigned* fr, unsigned nf, int sys, int crc,
                           const float* llr, unsigned long F, float* soft, float* ext, unsigned char* info,
                           unsigned char* ok)
{
    std::vector<unsigned> frozen(fr, fr + nf);
    Decoding::Scan* dec = new Decoding::Scan(N, it, frozen);
    ErrorDetection::Detector* det = ErrorDetection::create(crc, "crc");
    dec->setSystematic(sys != 0);
    dec->setErrorDetection(det);
    const unsigned long kb = (N - nf + 7) / 8;
    std::vector<unsigned char> buf(kb + 8);
    double secs = 0;
    for (unsigned long f = 0; f < F; ++f) {
        const auto t0 = std::chrono::steady_clock::now();
        const bool r = dec->decode_vector(llr + f * N, buf.data());
        secs += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        ok[f] = r ? 1 : 0;
        for (unsigned long b = 0; b < kb; ++b)
            info[f * kb + b] = buf[b];
        dec->getSoftCodeword(soft + f * N);
        dec->getExtrinsicChannelInformation(ext + f * N);
    }
    delete dec;
    delete det;
    return secs;
}
"""


def build_shim(tmp):
    import torch
    fmt = os.path.join(os.path.dirname(torch.__file__), "include")
    src, so = os.path.join(tmp, "scan_shim.cpp"), os.path.join(tmp, "libscanshim.so")
    with open(src, "w") as fh:
        fh.write(SHIM)
    subprocess.run(["g++", "-std=c++17", "-O2", "-mavx2", "-mfma", "-fPIC", "-shared", "-w", "-DFMT_HEADER_ONLY",
                    "-I", os.path.join(REF, "include"), "-isystem", fmt, src, "-o", so, "-L", REF_SO_DIR,
                    "-lpolarref", f"-Wl,-rpath,{REF_SO_DIR}"], check=True)
    lib = C.CDLL(so)
    P = C.c_void_p
    lib.scan_ref.argtypes = [C.c_uint, C.c_uint, P, C.c_uint, C.c_int, C.c_int, P, C.c_ulong, P, P, P, P]
    lib.scan_ref.restype = C.c_double
    return lib


def ref_scan(lib, N, it, frozen, llr, systematic=True, crc=8):
    fr = np.ascontiguousarray(np.asarray(list(frozen), np.uint32))
    llr = np.ascontiguousarray(llr, np.float32).reshape(-1, N)
    F, kb = llr.shape[0], (N - fr.size + 7) // 8
    soft, ext = np.zeros((F, N), np.float32), np.zeros((F, N), np.float32)
    info, ok = np.zeros((F, kb), np.uint8), np.zeros(F, np.uint8)
    secs = lib.scan_ref(N, it, fr.ctypes.data, fr.size, int(systematic), crc, llr.ctypes.data, F, soft.ctypes.data,
                        ext.ctypes.data, info.ctypes.data, ok.ctypes.data)
    return soft, ext, info, ok, secs


def main():
    rng = np.random.default_rng(20261019)
    fx = {}
    with tempfile.TemporaryDirectory() as tmp:
        lib = build_shim(tmp)
        # the reference's own known-answer frame (decodingtest.cpp: N = 8, frozen {0, 1, 2, 4})
        kat = np.array([[-5, -6, -4, 1, -4, -5, -7, 2]], np.float32)
        codes = [(8, [0, 1, 2, 4], kat)]  # (N, frozen, llr), shared by the cases of a code
        cases = []  # (code, iterations, systematic)
        for it in (1, 2):
            for sysm in (1, 0):
                cases.append((0, it, sysm))
        sets = [(N, frozen_bits(N, K, 0.0)) for N, K in ((16, 8), (64, 32), (256, 64), (256, 192))]
        for N in (64, 128):
            K = int(rng.integers(N // 4, 3 * N // 4))
            sets.append((N, sorted(rng.choice(N, N - K, replace=False).tolist())))
        for N, fr in sets:
            codes.append((N, fr, np.concatenate([llr_kinds(rng, 2, N, k) for k in LLR_KINDS])))
            for it in (1, 2, 4):
                for sysm in (1, 0):
                    cases.append((len(codes) - 1, it, sysm))
        N = 1024
        codes.append((N, frozen_bits(N, 512, 0.0), np.concatenate([llr_kinds(rng, 2, N, k) for k in LLR_KINDS])))
        cases.append((len(codes) - 1, 4, 1))
        for j, (N, fr, llr) in enumerate(codes):
            fx[f"code{j}_frozen"] = np.array(fr, np.uint16)
            fx[f"code{j}_llr"] = llr
        meta = []
        for i, (j, it, sysm) in enumerate(cases):
            N, fr, llr = codes[j]
            soft, ext, info, ok, _ = ref_scan(lib, N, it, fr, llr, bool(sysm), 8)
            assert not np.isnan(soft).any() and not np.isnan(ext).any()
            meta.append([N, j, it, sysm])
            fx[f"c{i}_soft"], fx[f"c{i}_ext"], fx[f"c{i}_info"], fx[f"c{i}_ok"] = soft, ext, info, ok
        fx["meta"] = np.array(meta, np.int32)  # per case: N, code, iterations, systematic
        # the reference's single-thread rate at (1024, 512), 4 iterations and 1
        N, fr = 1024, frozen_bits(1024, 512, 0.0)
        llr = llr_kinds(rng, 1024, N, "normal")
        rates = []
        for it in (4, 1):
            ref_scan(lib, N, it, fr, llr[:64])
            rates.append(llr.shape[0] / ref_scan(lib, N, it, fr, llr)[4])
        fx["ref_cw_per_s"] = np.array(rates, np.float64)  # [4 iterations, 1 iteration]
    out = os.path.join(HERE, "scan_fixtures.npz")
    np.savez_compressed(out, **fx)
    print(f"wrote {out} ({os.path.getsize(out) // 1024} KiB), {len(cases)} cases, "
          f"reference {rates[0]:.3g} cw/s at 4 iterations, {rates[1]:.3g} at 1")


if __name__ == "__main__":
    main()
