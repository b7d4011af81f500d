"""numpy restatement of the reference's SCAN decoder (src/polarcode/decoding/scan.cpp), vectorised
over frames.  Test code: the checker of tests/test_gpu_scan.py, pinned to the reference's own
outputs by tests/test_scan_restatement.py.  The product never imports it.

It follows scan.cpp statement for statement (the group loop, updatellrmap, updatebitmap, the
index functions), not the kernel's schedule: every value has the reference's fp32 expression.
"""
import numpy as np

_SIGN = np.uint32(0x80000000)


def _f(a, b):
    """F_function_calc (templatized_float.h:85-90): fmin(|a|, |b|) with sign bit sign(a) ^ sign(b)."""
    m = np.fmin(np.abs(a), np.abs(b)).astype(np.float32)
    s = (np.ascontiguousarray(a).view(np.uint32) ^ np.ascontiguousarray(b).view(np.uint32)) & _SIGN
    return (m.view(np.uint32) | s).view(np.float32)


def bit_reverse(n):
    """bit_reverse(i, n) of scan.cpp:212-221 for i = 0 .. 2^n - 1."""
    i = np.arange(1 << n)
    r = np.zeros_like(i)
    for b in range(n):
        r |= ((i >> b) & 1) << (n - 1 - b)
    return r


def scan_decode(N, frozen, llr, iterations, systematic=True):
    """Scan::decode over F frames: returns (soft codeword F x N, extrinsic F x N, info bytes
    F x ceil(K/8)), float32 bit patterns as the reference's."""
    llr = np.ascontiguousarray(llr, np.float32).reshape(-1, N)
    F, n = llr.shape[0], N.bit_length() - 1
    isf = np.zeros(N, bool)
    isf[np.asarray(list(frozen), int)] = True
    L = np.zeros((F, 2 * N - 1), np.float32)
    E = np.zeros((F, 2 * N - 1), np.float32)
    O = np.zeros((F, (n + 1) * N // 2), np.float32)
    out = np.zeros((F, N), np.float32)  # mSystematicOutput
    br = bit_reverse(n)
    inf = np.float32(np.inf)

    def ev(level):  # evenIndex(n, level, 0)
        return (1 << (n + 1)) - (1 << (n + 1 - level))

    def od(level, group):  # oddIndex(n, level, group, 0)
        if level == n:
            return (group >> 1) + ((level - 1) << (n - 1))
        return ((group - 1) << (n - 1 - level)) + ((level - 1) << (n - 1))

    def updatellrmap(level, group):
        if level == 0:
            return
        if (group & 1) == 0:
            updatellrmap(level - 1, group // 2)
        gs = 1 << (n - level)
        p, c = ev(level - 1), ev(level)
        a, b = L[:, p:p + 2 * gs:2], L[:, p + 1:p + 2 * gs:2]
        if group & 1:
            L[:, c:c + gs] = b + _f(a, E[:, c:c + gs])
        else:
            o = od(level, group + 1)
            L[:, c:c + gs] = _f(a, b + O[:, o:o + gs])

    def updatebitmap(level, group):
        while group & 1:
            left = group // 2
            gs = 1 << (n - level)
            p, c, o = ev(level - 1), ev(level), od(level, group)
            a, b = L[:, p:p + 2 * gs:2], L[:, p + 1:p + 2 * gs:2]
            Oc, Ec = O[:, o:o + gs], E[:, c:c + gs]
            u0 = _f(Ec, Oc + b)
            u1 = Oc + _f(Ec, a)
            if left & 1:
                d = od(level - 1, left)
                O[:, d:d + 2 * gs:2] = u0
                O[:, d + 1:d + 2 * gs:2] = u1
            else:
                E[:, p:p + 2 * gs:2] = u0
                E[:, p + 1:p + 2 * gs:2] = u1
                return
            level, group = level - 1, left

    L[:, br] = llr  # mLlr[evenIndex(0, bit_reverse(i))] = channel[i]
    for i in range(1, N, 2):
        if isf[i]:
            O[:, od(n, i)] = inf
    for _ in range(iterations):
        for group in range(N):
            updatellrmap(n, group)
            out[:, group] = L[:, ev(n)]
            if group & 1:
                out[:, group] += O[:, od(n, group)]
                updatebitmap(n, group)
            else:
                E[:, ev(n)] = inf if isf[group] else np.float32(0.0)
                out[:, group] += E[:, ev(n)]
    if systematic:
        soft = (L[:, :N] + E[:, :N])[:, br]
    else:
        soft = out[:, br]
    ext = E[:, :N][:, br]
    bits = (np.ascontiguousarray(soft).view(np.uint32) >> 31).astype(np.uint8)[:, ~isf]
    return np.ascontiguousarray(soft), np.ascontiguousarray(ext), np.packbits(bits, axis=1)
