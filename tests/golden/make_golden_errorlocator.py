#!/usr/bin/env python3
"""Generate tests/golden/errorlocator_fixtures.npz from the REFERENCE's error locator.

Runs only where oracle/_ref/libpolarref.so was built from /root/reference's sources
(`make -C oracle ref`).  A small C++ shim of our own (below) is compiled into a temporary
directory against the reference's headers and that library (and, for the statistics, together with
the reference's src/errorlocator/statistics.cpp, which compiles on its own); it constructs
`new Decoding::ErrorLocator(N, frozen)` and records, per frame, getOutput(), getSoftCodeword,
firstError() and correctionCount() for setAsReferenceDecoder() + decode(), for plain decode() and
for decodeFindFirstError().  Nothing compiled is kept.  Data only: inputs and the reference's
outputs.  tests/test_errorlocator_restatement.py pins tests/errorlocator_numpy.py to these
fixtures; tests/test_gpu_errorlocator.py checks the HIP kernel against both.  Before anything is
written, both restatements must reproduce all of it.  No frame is dropped: nothing is ambiguous.

In reference mode the reference leaves firstError() / correctionCount() as they were (never set in
a fresh decoder); the fixtures record -1 and 0 there, which is what the C ABI defines.

    python tests/golden/make_golden_errorlocator.py
"""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

from errorlocator_numpy import MODES, frozen_mask, locate, locate_literal, statistics  # noqa: E402
from helpers import LLR_KINDS, llr_kinds  # noqa: E402

from antpolarcodes_amd import frames  # noqa: E402
from antpolarcodes_amd.construction import frozen_bits  # noqa: E402

REF = "/root/reference"
REF_SO_DIR = os.path.join(ROOT, "oracle", "_ref")

SHIM = r"""
#include <polarcode/decoding/errorlocator.h>
#include "statistics.h"
#include <chrono>
#include <cstring>
#include <sstream>
#include <vector>
using namespace PolarCode;
// F frames through one ErrorLocator.  mode 0: setAsReferenceDecoder() + decode(); 1: decode();
// 2: decodeFindFirstError().  desired may be null (the decoder's defaults stay).  Returns the
// seconds the decode calls took.
extern "C" double el_ref(unsigned N, const unsigned* fr, unsigned nf, int mode, const float* llr, const float* desired,
                         unsigned long F, float* u, float* words, int* first, int* count)
{
    std::vector<unsigned> frozen(fr, fr + nf);
    Decoding::ErrorLocator* dec = new Decoding::ErrorLocator(N, frozen);
    if (mode == 0)
        dec->setAsReferenceDecoder();
    double secs = 0;
    for (unsigned long f = 0; f < F; ++f) {
        dec->setSignal(llr + f * N);
        if (desired)
            dec->setDesiredOutput(std::vector<float>(desired + f * N, desired + f * N + N));
        const auto t0 = std::chrono::steady_clock::now();
        int ff = -1;
        if (mode == 2)
            ff = dec->decodeFindFirstError();
        else
            dec->decode();
        secs += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        first[f] = mode == 0 ? -1 : mode == 2 ? ff : dec->firstError();
        count[f] = mode == 0 ? 0 : dec->correctionCount();
        const std::vector<float> out = dec->getOutput();
        std::memcpy(u + f * N, out.data(), N * sizeof(float));
        dec->getSoftCodeword(words + f * N);
    }
    delete dec;
    return secs;
}
// Statistics::evaluate of n values: out = mean, dev, min, max, sum; str = the four CSV columns
// (mean, dev, min, max) as `file << float` writes them, 32 bytes each.
extern "C" void el_stats(const float* v, unsigned n, float* out, char* str)
{
    SimulationErrorLocator::Statistics s;
    for (unsigned i = 0; i < n; ++i)
        s.insert(v[i]);
    SimulationErrorLocator::StatisticsOutput r = s.evaluate();
    const float cols[5] = { r.mean, r.dev, r.min, r.max, r.sum };
    std::memcpy(out, cols, sizeof cols);
    for (int i = 0; i < 4; ++i) {
        std::ostringstream os;
        os << cols[i];
        std::strncpy(str + 32 * i, os.str().c_str(), 31);
    }
}
"""


def build_shim(tmp):
    import torch
    fmt = os.path.join(os.path.dirname(torch.__file__), "include")
    src, so = os.path.join(tmp, "el_shim.cpp"), os.path.join(tmp, "libelshim.so")
    with open(src, "w") as fh:
        fh.write(SHIM)
    stat = os.path.join(REF, "src", "errorlocator")
    subprocess.run(["g++", "-std=c++17", "-O2", "-mavx2", "-mfma", "-fPIC", "-shared", "-w", "-DFMT_HEADER_ONLY",
                    "-I", os.path.join(REF, "include"), "-I", stat, "-isystem", fmt, src,
                    os.path.join(stat, "statistics.cpp"), "-o", so, "-L", REF_SO_DIR, "-lpolarref",
                    f"-Wl,-rpath,{REF_SO_DIR}"], check=True)
    lib = C.CDLL(so)
    P = C.c_void_p
    lib.el_ref.argtypes = [C.c_uint, P, C.c_uint, C.c_int, P, P, C.c_ulong, P, P, P, P]
    lib.el_ref.restype = C.c_double
    lib.el_stats.argtypes = [P, C.c_uint, P, P]
    lib.el_stats.restype = None
    return lib


def ref_locate(lib, N, frozen, llr, desired, mode):
    fr = np.ascontiguousarray(np.asarray(list(frozen), np.uint32))
    llr = np.ascontiguousarray(llr, np.float32).reshape(-1, N)
    F = llr.shape[0]
    if desired is not None:
        desired = np.ascontiguousarray(desired, np.float32).reshape(F, N)
    u, words = np.zeros((F, N), np.float32), np.zeros((F, N), np.uint32)
    first, count = np.zeros(F, np.int32), np.zeros(F, np.int32)
    secs = lib.el_ref(N, fr.ctypes.data, fr.size, MODES.index(mode), llr.ctypes.data,
                      None if desired is None else desired.ctypes.data, F, u.ctypes.data, words.ctypes.data,
                      first.ctypes.data, count.ctypes.data)
    return u, words, first, count.astype(np.uint32), secs


def ref_stats(lib, values):
    v = np.ascontiguousarray(values, np.float32)
    out, buf = np.zeros(5, np.float32), C.create_string_buffer(128)
    lib.el_stats(v.ctypes.data if v.size else None, v.size, out.ctypes.data, buf)
    return out, [buf.raw[32 * i:32 * i + 32].split(b"\0")[0].decode() for i in range(4)]


def same(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8),
                                                 np.ascontiguousarray(b).view(np.uint8))


def noisy_pair(N, fr, F, sigma, seed):
    """(noisy BPSK scaled by 4, the noiseless +-1 signal) of F non-systematic codewords."""
    x = frames.awgn_frames(N, fr, F, 2.0, seed=seed, crc=0, systematic=False)[2]
    clean = (1.0 - 2.0 * x.astype(np.float32)).astype(np.float32)
    rng = np.random.default_rng(seed + 1000)
    noisy = (np.float32(4.0) * (clean + np.float32(sigma) * rng.standard_normal((F, N)).astype(np.float32)))
    return noisy.astype(np.float32), clean


def arbitrary_desired(rng, F, N):
    """Random signs and magnitudes at all N positions, signed zeros and infinities among them."""
    d = (rng.normal(0, 1, (F, N)) * 10.0 ** rng.uniform(-2, 2, (F, N))).astype(np.float32)
    d[rng.random((F, N)) < 0.1] = 0.0
    d[rng.random((F, N)) < 0.1] = -0.0
    d[rng.random((F, N)) < 0.05] = np.inf
    return d


def main():
    rng = np.random.default_rng(20261022)
    fx = {}
    with tempfile.TemporaryDirectory() as tmp:
        lib = build_shim(tmp)
        codes, cases = [], []  # codes: (N, frozen); cases: (code, llr, desired or None)

        def code(N, fr):
            codes.append((N, list(fr)))
            return len(codes) - 1

        def crafted(j, llr):
            """Desired vectors made from the frames' own reference-mode outputs: unchanged (no
            correction), and with the sign flipped at the first / the last information bit."""
            N, fr = codes[j]
            info = np.flatnonzero(~frozen_mask(N, fr))
            own = locate(N, fr, llr, None, "reference")[0]
            out = [own.copy()]
            for i in (info[0], info[-1]):
                d = own.copy()
                d[:, i] = -d[:, i]
                out.append(d)
            return np.concatenate([llr] * 3), np.concatenate(out)

        # the reference's own known-answer frame (decodingtest.cpp: N = 8, frozen {0, 1, 2, 4})
        j = code(8, [0, 1, 2, 4])
        kat = np.array([[-5, -6, -4, 1, -4, -5, -7, 2]], np.float32)
        cases.append((j, kat, None))
        cases.append((j, np.concatenate([kat, llr_kinds(rng, 3, 8, "zeros")]), arbitrary_desired(rng, 4, 8)))
        cases.append((j, *crafted(j, llr_kinds(rng, 1, 8, "normal"))))
        sizes = (((16, 8), 2, 3), ((64, 32), 2, 3), ((256, 64), 1, 2), ((256, 192), 1, 2), ((1024, 512), 1, 1))
        for (N, K), nk, na in sizes:
            fr = frozen_bits(N, K, 0.0)
            j = code(N, fr)
            # every LLR kind against the defaults (+0 at information bits: signed zeros matter)
            cases.append((j, np.concatenate([llr_kinds(rng, nk, N, k) for k in LLR_KINDS]), None))
            # the tool's use: desired = the reference-mode output on the noiseless signal
            for sigma in (0.6, 0.9):
                noisy, clean = noisy_pair(N, fr, na, sigma, seed=N + K + int(10 * sigma))
                des = ref_locate(lib, N, fr, clean, None, "reference")[0]
                cases.append((j, noisy, des))
            # arbitrary desired vectors, negative values at frozen positions among them
            nc = 1 if N >= 1024 else 2
            cases.append((j, np.concatenate([llr_kinds(rng, nc, N, "normal"), llr_kinds(rng, nc, N, "zeros")]),
                          arbitrary_desired(rng, 2 * nc, N)))
            if N <= 64:
                cases.append((j, *crafted(j, llr_kinds(rng, 1, N, "normal"))))
        for N in (32, 64):  # two random frozen sets
            K = int(rng.integers(N // 4, 3 * N // 4))
            fr = sorted(rng.choice(N, N - K, replace=False).tolist())
            j = code(N, fr)
            cases.append((j, np.concatenate([llr_kinds(rng, 1, N, k) for k in LLR_KINDS]), None))
            cases.append((j, llr_kinds(rng, 4, N, "wide"), arbitrary_desired(rng, 4, N)))
            cases.append((j, *crafted(j, llr_kinds(rng, 1, N, "zeros"))))
        j = code(16, [0])  # K = N - 1
        cases.append((j, np.concatenate([llr_kinds(rng, 1, 16, k) for k in LLR_KINDS]), None))
        cases.append((j, llr_kinds(rng, 3, 16, "ints"), arbitrary_desired(rng, 3, 16)))

        for j, (N, fr) in enumerate(codes):
            fx[f"code{j}_frozen"] = np.array(fr, np.uint16)
        meta, counts, spots = [], [], set()
        for i, (j, llr, des) in enumerate(cases):
            N, fr = codes[j]
            info = np.flatnonzero(~frozen_mask(N, fr))
            fx[f"c{i}_llr"] = llr
            if des is not None:
                fx[f"c{i}_desired"] = des
            for mode in MODES:
                u, words, first, count, _ = ref_locate(lib, N, fr, llr, des, mode)
                # both restatements reproduce what is about to be written
                for form in (locate, locate_literal):
                    want = form(N, fr, llr, des, mode)
                    assert same(want[0], u) and same(want[1], words) and same(want[2], first) and \
                        same(want[3], count), (i, N, mode, form.__name__)
                fx[f"c{i}_{mode}_u"], fx[f"c{i}_{mode}_bits"] = u, words
                fx[f"c{i}_{mode}_first"], fx[f"c{i}_{mode}_count"] = first, count
                if mode == "correct":
                    counts += count.tolist()
                    spots |= {"first8"} if ((first >= 0) & (first // 8 == info[0] // 8)).any() else set()
                    spots |= {"last8"} if ((first >= 0) & (first // 8 == info[-1] // 8)).any() else set()
            meta.append([N, j, llr.shape[0], int(des is not None)])
        counts = np.array(counts)
        assert (counts == 0).any() and (counts == 1).any() and (counts >= 64).any(), np.bincount(counts)
        assert spots == {"first8", "last8"}, spots
        fx["meta"] = np.array(meta, np.int32)  # per case: N, code, frames, has a desired vector

        # Statistics::evaluate: sizes 0, 1, 2; a descending run, where the `else if` never looks
        # at the maximum branch; a minimum that is also tested against the maximum; many values
        seqs = [[], [3], [2, 5], [9, 7, 4, 1], [4, 1, 8, 8, 2], [1, 1, 1], rng.integers(1, 203, 57).tolist(),
                [202, 1, 17, 64, 3, 3, 120]]
        for k, s in enumerate(seqs):
            out, strs = ref_stats(lib, s)
            got = statistics(s)
            assert same(np.array(got, np.float32), out), (k, got, out)
            fx[f"stat{k}_values"], fx[f"stat{k}_out"] = np.array(s, np.float32), out
            fx[f"stat{k}_str"] = np.array(strs)
        fx["stat_count"] = np.array([len(seqs)], np.int32)

        # the reference's single-thread rate at (1024, 512) on the frames scan_time locates
        N, fr = 1024, frozen_bits(1024, 512, 0.0)
        llr, _, x = frames.awgn_frames(N, fr, 1024, 2.0, seed=1, crc=8)
        des = ref_locate(lib, N, fr, (1.0 - 2.0 * x.astype(np.float32)).astype(np.float32), None, "reference")[0]
        ref_locate(lib, N, fr, llr[:64], des[:64], "correct")
        runs = [ref_locate(lib, N, fr, llr, des, "correct") for _ in range(3)]
        rate = max(llr.shape[0] / r[4] for r in runs)
        fx["ref_cw_per_s"] = np.array([rate], np.float64)
        fx["ref_mean_corrections"] = np.array([runs[0][3].mean()], np.float64)
    out = os.path.join(HERE, "errorlocator_fixtures.npz")
    np.savez_compressed(out, **fx)
    print(f"wrote {out} ({os.path.getsize(out) // 1024} KiB), {len(cases)} cases, corrections up to {counts.max()}, "
          f"reference {rate:.3g} cw/s at {runs[0][3].mean():.3g} mean corrections")


if __name__ == "__main__":
    main()
