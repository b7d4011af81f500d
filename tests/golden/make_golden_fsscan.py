#!/usr/bin/env python3
"""Generate tests/golden/fsscan_fixtures.npz from the REFERENCE's Fast-SSCAN decoder.

Runs only where oracle/_ref/libpolarref.so was built from /root/reference's sources
(`make -C oracle ref`).  A small C++ shim of our own (below) is compiled into a temporary
directory against the reference's headers and that library; it constructs
`new Decoding::FastSscanFloat(N, trialLimit, frozen)` and records decode_vector, optional
decodeAgain() calls and getSoftCodeword.  Nothing compiled is kept.  Data only: inputs and the
reference's outputs.  tests/test_fsscan_restatement.py pins tests/fsscan_numpy.py to these
fixtures; tests/test_gpu_fsscan.py checks the HIP kernel against both.  Before anything is
written, the restatement must reproduce all of it.

    python tests/golden/make_golden_fsscan.py
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

from fsscan_numpy import fsscan_census, fsscan_decode  # noqa: E402
from helpers import LLR_KINDS, llr_kinds  # noqa: E402
from pyoracle import Oracle  # noqa: E402

from antpolarcodes_amd import frames  # noqa: E402
from antpolarcodes_amd.construction import frozen_bits  # noqa: E402

REF = "/root/reference"
REF_SO_DIR = os.path.join(ROOT, "oracle", "_ref")

SHIM = r"""
#include <polarcode/decoding/fastsscan_float.h>
#include <polarcode/errordetection/errordetector.h>
#include <chrono>
#include <vector>
using namespace PolarCode;
// F frames through one FastSscanFloat decoder (fresh != 0: a new decoder per frame); `again`
// decodeAgain() calls follow each decode.  Returns the seconds the decode calls took.
extern "C" double fss_ref(unsigned N, unsigned limit, const unsigned* fr, unsigned nf, int crc, int again, int fresh,
                          const float* llr, unsigned long F, float* soft, unsigned char* info, unsigned char* ok)
{
    std::vector<unsigned> frozen(fr, fr + nf);
    ErrorDetection::Detector* det = ErrorDetection::create(crc, "crc");
    Decoding::FastSscanFloat* dec = nullptr;
    const unsigned long kb = (N - nf + 7) / 8;
    std::vector<unsigned char> buf(kb + 8);
    double secs = 0;
    for (unsigned long f = 0; f < F; ++f) {
        if (!dec || fresh) {
            delete dec;
            dec = new Decoding::FastSscanFloat(N, limit, frozen);
            dec->setErrorDetection(det);
        }
        const auto t0 = std::chrono::steady_clock::now();
        bool r = dec->decode_vector(llr + f * N, buf.data());
        for (int k = 0; k < again; ++k)
            r = dec->decodeAgain();
        secs += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (again)
            dec->getDecodedInformationBits(buf.data());
        ok[f] = r ? 1 : 0;
        for (unsigned long b = 0; b < kb; ++b)
            info[f * kb + b] = buf[b];
        dec->getSoftCodeword(soft + f * N);
    }
    delete dec;
    delete det;
    return secs;
}
"""


def build_shim(tmp):
    import torch
    fmt = os.path.join(os.path.dirname(torch.__file__), "include")
    src, so = os.path.join(tmp, "fss_shim.cpp"), os.path.join(tmp, "libfssshim.so")
    with open(src, "w") as fh:
        fh.write(SHIM)
    subprocess.run(["g++", "-std=c++17", "-O2", "-mavx2", "-mfma", "-fPIC", "-shared", "-w", "-DFMT_HEADER_ONLY",
                    "-I", os.path.join(REF, "include"), "-isystem", fmt, src, "-o", so, "-L", REF_SO_DIR,
                    "-lpolarref", f"-Wl,-rpath,{REF_SO_DIR}"], check=True)
    lib = C.CDLL(so)
    P = C.c_void_p
    lib.fss_ref.argtypes = [C.c_uint, C.c_uint, P, C.c_uint, C.c_int, C.c_int, C.c_int, P, C.c_ulong, P, P, P]
    lib.fss_ref.restype = C.c_double
    return lib


def ref_fsscan(lib, N, limit, frozen, llr, crc=8, again=0, fresh=False):
    fr = np.ascontiguousarray(np.asarray(list(frozen), np.uint32))
    llr = np.ascontiguousarray(llr, np.float32).reshape(-1, N)
    F, kb = llr.shape[0], (N - fr.size + 7) // 8
    soft = np.zeros((F, N), np.float32)
    info, ok = np.zeros((F, kb), np.uint8), np.zeros(F, np.uint8)
    secs = lib.fss_ref(N, limit, fr.ctypes.data, fr.size, crc, again, int(fresh), llr.ctypes.data, F,
                       soft.ctypes.data, info.ctypes.data, ok.ctypes.data)
    return soft, info, ok, secs


def ref_trials(lib, N, limit, frozen, llr, crc):
    """Passes decode() ran per frame: the first t <= limit at which a fresh decoder of limit t
    reports success, else limit."""
    tr = np.full(llr.shape[0], limit, np.uint8)
    for t in range(limit - 1, 0, -1):
        tr[ref_fsscan(lib, N, t, frozen, llr, crc, fresh=True)[2] != 0] = t
    return tr


def same(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8),
                                                 np.ascontiguousarray(b).view(np.uint8))


def main():
    rng = np.random.default_rng(20261020)
    orc = Oracle()
    fx = {}
    with tempfile.TemporaryDirectory() as tmp:
        lib = build_shim(tmp)
        # the reference's own known-answer frame (decodingtest.cpp:1259-1272: N = 8, frozen
        # {0, 1, 2, 4}, trial limit 1, no detector), as decode() and as decode() + decodeAgain()
        kat = np.array([[-5, -6, -4, 1, -4, -5, -7, 2]], np.float32)
        codes = [(8, [0, 1, 2, 4], kat)]  # (N, frozen, llr), shared by the cases of a code
        cases = [(0, 1, 0, 0, 0), (0, 1, 0, 1, 0)]  # (code, limit, crc, decodeAgain calls, reused decoder)
        for (N, K), nk, na in (((16, 8), 2, 6), ((64, 32), 2, 6), ((256, 64), 1, 5), ((256, 192), 1, 5),
                               ((1024, 512), 1, 3)):
            fr = frozen_bits(N, K, 0.0)
            assert fsscan_census(N, fr)["right_twobit"] == 0
            llr = np.concatenate([llr_kinds(rng, nk, N, k) for k in LLR_KINDS] +
                                 [frames.awgn_frames(N, fr, na, 1.5, seed=N + K, crc=8)[0]])
            codes.append((N, fr, llr))
            for limit in (1, 2, 4):
                cases.append((len(codes) - 1, limit, 8, 0, 0))
        # two random sets with a TwoBit node that is a right child, through ONE reused decoder
        for N in (32, 64):
            while True:
                K = int(rng.integers(N // 4, 3 * N // 4))
                fr = sorted(rng.choice(N, N - K, replace=False).tolist())
                if fsscan_census(N, fr)["right_twobit"] >= 2:
                    break
            codes.append((N, fr, np.concatenate([llr_kinds(rng, 2, N, k) for k in LLR_KINDS])))
            cases.append((len(codes) - 1, 2, 0, 0, 1))
            cases.append((len(codes) - 1, 3, 8, 0, 1))
        for j, (N, fr, llr) in enumerate(codes):
            fx[f"code{j}_frozen"] = np.array(fr, np.uint16)
            fx[f"code{j}_llr"] = llr
        meta = []
        for i, (j, limit, crc, again, reused) in enumerate(cases):
            N, fr, llr = codes[j]
            soft, info, ok, _ = ref_fsscan(lib, N, limit, fr, llr, crc, again, fresh=not reused)
            assert not np.isnan(soft).any()
            # the restatement reproduces what is about to be written
            chk = (lambda row, c=crc: orc.crc(c, row)) if crc else None
            want = fsscan_decode(N, fr, llr, limit + again, chk, carry=bool(reused), forced=bool(again))
            assert same(want[0], soft) and same(want[1], info) and same(want[2], ok), (i, N, limit, crc, again)
            if reused:  # the first frame of a reused decoder = the zero start
                zero = fsscan_decode(N, fr, llr[:1], limit, chk)
                assert same(zero[0], soft[:1]) and same(zero[1], info[:1])
                tr = want[3]
            elif again:
                tr = np.full(llr.shape[0], limit + again, np.uint8)
            else:
                tr = ref_trials(lib, N, limit, fr, llr, crc)
                assert same(want[3], tr), (i, want[3], tr)
            meta.append([N, j, limit, crc, again, reused])
            fx[f"c{i}_soft"], fx[f"c{i}_info"], fx[f"c{i}_ok"], fx[f"c{i}_trials"] = soft, info, ok, tr
        fx["meta"] = np.array(meta, np.int32)  # per case: N, code, limit, crc, decodeAgain calls, reused
        # the reference's single-thread rate at (1024, 512), CRC-8, the frames scan_time decodes
        N, fr = 1024, frozen_bits(1024, 512, 0.0)
        llr = frames.awgn_frames(N, fr, 1024, 2.0, seed=1, crc=8)[0]
        rates = []
        for limit in (1, 4):
            ref_fsscan(lib, N, limit, fr, llr[:64])
            rates.append(max(llr.shape[0] / ref_fsscan(lib, N, limit, fr, llr)[3] for _ in range(5)))
        fx["ref_cw_per_s"] = np.array(rates, np.float64)  # [limit 1, limit 4]
    out = os.path.join(HERE, "fsscan_fixtures.npz")
    np.savez_compressed(out, **fx)
    print(f"wrote {out} ({os.path.getsize(out) // 1024} KiB), {len(cases)} cases, "
          f"reference {rates[0]:.3g} cw/s at limit 1, {rates[1]:.3g} at limit 4")


if __name__ == "__main__":
    main()
