#!/usr/bin/env python3
"""Generate tests/golden/depthfirst_fixtures.npz from the REFERENCE's SC-Flip decoder.

Runs only where oracle/_ref/libpolarref.so was built from /root/reference's sources
(`make -C oracle ref`).  A small C++ shim of our own (below) is compiled into a temporary
directory against the reference's headers and that library; it constructs
`new Decoding::DepthFirst(N, trialLimit, frozen)`, sets the detector and records decode_vector,
getDecodedInformationBits and getSoftCodeword.  Nothing compiled is kept.  Data only: inputs and
the reference's outputs.  tests/test_depthfirst_restatement.py pins tests/depthfirst_numpy.py to
these fixtures; tests/test_gpu_depthfirst.py checks the HIP kernel against both.  Before anything
is written, the restatement must reproduce all of it.

The trials a frame ran are counted, not inferred: the shim's detector wraps the reference's and
counts its check() calls, one per trial (DepthFirst::decode).  A fresh decoder of a smaller limit
would not do: Manager::decode's initial queue depends on the limit itself (the 2T/3 rule), so
trial t of a limit-T decoder is not trial t of a limit-t decoder.

At T > 1 only frames whose search met no tie are comparable with the reference (std::sort's order
among equal reliabilities is libstdc++'s): inputs are the continuous LLR kinds and
AWGN frames, and frames the restatement flags ambiguous are dropped (asserted below 5 %).

    python tests/golden/make_golden_depthfirst.py
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

from depthfirst_numpy import depthfirst_decode  # noqa: E402
from helpers import LLR_KINDS, llr_kinds  # noqa: E402
from pyoracle import Oracle  # noqa: E402

from antpolarcodes_amd import frames  # noqa: E402
from antpolarcodes_amd.construction import frozen_bits  # noqa: E402

REF = "/root/reference"
REF_SO_DIR = os.path.join(ROOT, "oracle", "_ref")

SHIM = r"""
#include <polarcode/decoding/depth_first.h>
#include <polarcode/errordetection/errordetector.h>
#include <chrono>
#include <vector>
using namespace PolarCode;
// the reference's detector, counting its check() calls: DepthFirst::decode checks once per trial
struct Counting : ErrorDetection::Detector {
    ErrorDetection::Detector* d;
    unsigned checks = 0;
    explicit Counting(ErrorDetection::Detector* p) : d(p) {}
    ~Counting() override { delete d; }
    unsigned getCheckBitCount() override { return d->getCheckBitCount(); }
    std::string getType() override { return d->getType(); }
    void generate(void* data, int bytes) override { d->generate(data, bytes); }
    bool check(void* data, int bytes) override { ++checks; return d->check(data, bytes); }
    int multiCheck(void** data, int n, int b) override { return d->multiCheck(data, n, b); }
};
// F frames through one DepthFirst decoder.  Returns the seconds the decode calls took.
extern "C" double df_ref(unsigned N, unsigned limit, const unsigned* fr, unsigned nf, int crc, int systematic,
                         const float* llr, unsigned long F, float* words, unsigned char* info, unsigned char* ok,
                         unsigned char* trials)
{
    std::vector<unsigned> frozen(fr, fr + nf);
    Counting det(ErrorDetection::create(crc, "crc"));
    Decoding::DepthFirst* dec = new Decoding::DepthFirst(N, limit, frozen);
    dec->setErrorDetection(&det);
    dec->setSystematic(systematic != 0);
    const unsigned long kb = (N - nf + 7) / 8;
    std::vector<unsigned char> buf(kb + 8);
    double secs = 0;
    for (unsigned long f = 0; f < F; ++f) {
        det.checks = 0;
        const auto t0 = std::chrono::steady_clock::now();
        const bool r = dec->decode_vector(llr + f * N, buf.data());
        secs += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        dec->getDecodedInformationBits(buf.data());
        ok[f] = r ? 1 : 0;
        trials[f] = (unsigned char)det.checks;
        for (unsigned long b = 0; b < kb; ++b)
            info[f * kb + b] = buf[b];
        dec->getSoftCodeword(words + f * N);
    }
    delete dec;
    return secs;
}
"""


def build_shim(tmp):
    import torch
    fmt = os.path.join(os.path.dirname(torch.__file__), "include")
    src, so = os.path.join(tmp, "df_shim.cpp"), os.path.join(tmp, "libdfshim.so")
    with open(src, "w") as fh:
        fh.write(SHIM)
    subprocess.run(["g++", "-std=c++17", "-O2", "-mavx2", "-mfma", "-fPIC", "-shared", "-w", "-DFMT_HEADER_ONLY",
                    "-I", os.path.join(REF, "include"), "-isystem", fmt, src, "-o", so, "-L", REF_SO_DIR,
                    "-lpolarref", f"-Wl,-rpath,{REF_SO_DIR}"], check=True)
    lib = C.CDLL(so)
    P = C.c_void_p
    lib.df_ref.argtypes = [C.c_uint, C.c_uint, P, C.c_uint, C.c_int, C.c_int, P, C.c_ulong, P, P, P, P]
    lib.df_ref.restype = C.c_double
    return lib


def ref_depthfirst(lib, N, limit, frozen, llr, crc=8, systematic=True):
    fr = np.ascontiguousarray(np.asarray(list(frozen), np.uint32))
    llr = np.ascontiguousarray(llr, np.float32).reshape(-1, N)
    F, kb = llr.shape[0], (N - fr.size + 7) // 8
    words = np.zeros((F, N), np.uint32)
    info, ok, tr = np.zeros((F, kb), np.uint8), np.zeros(F, np.uint8), np.zeros(F, np.uint8)
    secs = lib.df_ref(N, limit, fr.ctypes.data, fr.size, crc, int(systematic), llr.ctypes.data, F,
                      words.ctypes.data, info.ctypes.data, ok.ctypes.data, tr.ctypes.data)
    return words, info, ok, tr, secs


def same(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8),
                                                 np.ascontiguousarray(b).view(np.uint8))


def main():
    rng = np.random.default_rng(20261021)
    orc = Oracle()
    fx = {}
    drawn = dropped = 0
    with tempfile.TemporaryDirectory() as tmp:
        lib = build_shim(tmp)
        codes, cases = [], []  # codes: (N, frozen, llr); cases: (code, limit, crc, systematic)

        def add(N, fr, llr, limits, crc=8, systematic=True):
            """One code and its cases; at limits > 1 the frames the restatement flags ambiguous at
            any of the limits are dropped first."""
            nonlocal drawn, dropped
            chk = (lambda row, c=crc: orc.crc(c, row)) if crc else None
            if max(limits) > 1:
                amb = np.zeros(llr.shape[0], bool)
                for T in limits:
                    amb |= depthfirst_decode(N, fr, llr, T, chk, systematic)[4]
                drawn += llr.shape[0]
                dropped += int(amb.sum())
                llr = llr[~amb]
            codes.append((N, fr, llr))
            cases.extend((len(codes) - 1, T, crc, systematic) for T in limits)

        # the reference's own known-answer frame (decodingtest.cpp: N = 8, frozen {0, 1, 2, 4}),
        # trial limit 1, no detector
        add(8, [0, 1, 2, 4], np.array([[-5, -6, -4, 1, -4, -5, -7, 2]], np.float32), [1], crc=0)
        for (N, K), nk, na in (((16, 8), 2, 6), ((64, 32), 2, 6), ((256, 64), 1, 2), ((256, 192), 1, 2),
                               ((1024, 512), 1, 1)):
            fr = frozen_bits(N, K, 0.0)
            # limit 1: no selection is observable, every kind is comparable
            add(N, fr, np.concatenate([llr_kinds(rng, nk, N, k) for k in LLR_KINDS]), [1])
            cont = np.concatenate([llr_kinds(rng, nk, N, k) for k in ("normal", "wide")] +
                                  [frames.awgn_frames(N, fr, na, 1.5, seed=N + K, crc=8)[0]])
            add(N, fr, cont, [T for T in (2, 3, 4, 8, 32) if K >= T])
        # the four outcomes of the search within one case: (64, 32), CRC-8, limit 32, AWGN frames
        # scaled so that the 2T/3-th weakest leaf lies above log(9) and depth-1 configurations are
        # reached (entries 22 ..)
        N, K, T = 64, 32, 32
        fr = frozen_bits(N, K, 0.0)
        pool = (frames.awgn_frames(N, fr, 6000, 2.5, seed=7, crc=8)[0] * np.float32(8.0)).astype(np.float32)
        st = {}
        _, _, pok, ptr, pamb = depthfirst_decode(N, fr, pool, T, lambda row: orc.crc(8, row), reduced=True, stats=st)
        ld = st["last_depth"]
        pick = []
        for name, sel in (("first", (ptr == 1)), ("depth0", (pok == 1) & (ptr > 1) & (ld == 0)),
                          ("depth1", (pok == 1) & (ld == 1)), ("never", (pok == 0) & (ptr == T) & (ld == 1))):
            idx = np.flatnonzero(sel & ~pamb)[:4]
            assert idx.size > 0, f"no frame of kind {name}: change Eb/N0 or the scale"
            print(f"  search outcomes: {name}: {int((sel & ~pamb).sum())} of {pool.shape[0]}")
            pick += idx.tolist()
        add(N, fr, pool[rng.permutation(pick)], [T, 8, 4])
        fx["mix_case"] = np.array([len(cases) - 3], np.int32)  # the limit-32 case of the mix
        # dummy detector, CRC-32, non-systematic
        fr = frozen_bits(64, 32, 0.0)
        add(64, fr, np.concatenate([llr_kinds(rng, 3, 64, "normal"), llr_kinds(rng, 3, 64, "wide")]), [1, 4], crc=0)
        fr = frozen_bits(256, 192, 0.0)
        add(256, fr, np.concatenate([llr_kinds(rng, 1, 256, "normal"),
                                     frames.awgn_frames(256, fr, 4, 3.0, seed=3, crc=32)[0]]), [1, 4, 8], crc=32)
        fr = frozen_bits(64, 32, 0.0)
        ns = np.concatenate([llr_kinds(rng, 2, 64, "normal"),
                             frames.awgn_frames(64, fr, 8, 2.0, seed=11, crc=8, systematic=False)[0]])
        add(64, fr, ns, [1, 4, 8], systematic=False)
        # two random frozen sets
        for N in (32, 64):
            K = int(rng.integers(N // 4, 3 * N // 4))
            fr = sorted(rng.choice(N, N - K, replace=False).tolist())
            add(N, fr, np.concatenate([llr_kinds(rng, 3, N, "normal"), llr_kinds(rng, 3, N, "wide"),
                                       frames.awgn_frames(N, fr, 4, 3.0, seed=N, crc=8)[0]]), [1, 3, 8])
        assert dropped * 20 < drawn, (dropped, drawn)
        for j, (N, fr, llr) in enumerate(codes):
            fx[f"code{j}_frozen"] = np.array(fr, np.uint16)
            fx[f"code{j}_llr"] = llr
        meta, kinds = [], set()
        for i, (j, limit, crc, systematic) in enumerate(cases):
            N, fr, llr = codes[j]
            words, info, ok, tr, _ = ref_depthfirst(lib, N, limit, fr, llr, crc, systematic)
            # the restatement (the literal queue) reproduces what is about to be written
            chk = (lambda row, c=crc: orc.crc(c, row)) if crc else None
            st = {}
            want = depthfirst_decode(N, fr, llr, limit, chk, systematic, stats=st)
            assert limit == 1 or not want[4].any()
            assert same(want[0], words) and same(want[1], info) and same(want[2], ok) and same(want[3], tr), \
                (i, N, limit, crc, systematic)
            if limit >= 4:
                kinds |= {"first"} if (tr == 1).any() else set()
                kinds |= {"depth0"} if ((ok == 1) & (tr > 1) & (st["last_depth"] == 0)).any() else set()
                kinds |= {"depth1"} if ((ok == 1) & (st["last_depth"] == 1)).any() else set()
                kinds |= {"never"} if ((ok == 0) & (tr == limit) & (st["last_depth"] == 1)).any() else set()
            meta.append([N, j, limit, crc, int(systematic)])
            fx[f"c{i}_bits"], fx[f"c{i}_info"], fx[f"c{i}_ok"], fx[f"c{i}_trials"] = words, info, ok, tr
            fx[f"c{i}_depth"] = st["last_depth"].astype(np.int8)  # of the last decoded configuration
        assert kinds == {"first", "depth0", "depth1", "never"}, kinds
        fx["meta"] = np.array(meta, np.int32)  # per case: N, code, limit, crc, systematic
        # the reference's single-thread rate at (1024, 512), CRC-8, the frames scan_time decodes
        N, fr = 1024, frozen_bits(1024, 512, 0.0)
        llr = frames.awgn_frames(N, fr, 1024, 2.0, seed=1, crc=8)[0]
        rates = []
        for limit in (1, 8):
            ref_depthfirst(lib, N, limit, fr, llr[:64])
            rates.append(max(llr.shape[0] / ref_depthfirst(lib, N, limit, fr, llr)[4] for _ in range(5)))
        fx["ref_cw_per_s"] = np.array(rates, np.float64)  # [limit 1, limit 8]
    out = os.path.join(HERE, "depthfirst_fixtures.npz")
    np.savez_compressed(out, **fx)
    print(f"wrote {out} ({os.path.getsize(out) // 1024} KiB), {len(cases)} cases, dropped {dropped} of {drawn} frames, "
          f"reference {rates[0]:.3g} cw/s at limit 1, {rates[1]:.3g} at limit 8")


if __name__ == "__main__":
    main()
