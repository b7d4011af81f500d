"""A float32 numpy model of the ASK stages around the channel (helper of the ask tests; no test here).

Written from the formulas, independent of the device code:

  constants   power accumulates symbol * symbol in float32 over the odd symbols < 2^b;
              nm = float32(sqrt(2.0 * power / limit)), pn = float32(1.0 / nm), both in double
  modulate    bits past n count as 0; per symbol m = 1, s = 0, and for its bits in order
              m *= (bit ? -1 : +1), s = 2 s + m; x = s * pn
  demodulate  a = y * nm, shift = 2^(b-1); for k = 0 .. b-1: out[k] = a, a = |a| - shift, shift *= 0.5
  scale       out[k] *= gain, only bit positions < n kept
"""
import numpy as np

f32 = np.float32


def constants(b):
    power = f32(0.0)
    limit = f32(1 << b)
    symbol = f32(1.0)
    while symbol < limit:
        power = f32(power + f32(symbol * symbol))
        symbol = f32(symbol + f32(2.0))
    nm = f32(np.sqrt(2.0 * float(power) / float(limit)))
    pn = f32(1.0 / float(nm))
    return nm, pn


def symbol_count(n, b):
    return -(-n // b)


def modulate(code, n, b):
    """code: F x n/8 uint8 (MSB-first) -> F x S float32 symbols."""
    F = code.shape[0]
    S = symbol_count(n, b)
    bits = np.zeros((F, S * b), np.uint8)
    bits[:, :n] = np.unpackbits(code, axis=1)[:, :n]
    bits = bits.reshape(F, S, b)
    _, pn = constants(b)
    m = np.ones((F, S), f32)
    s = np.zeros((F, S), f32)
    for k in range(b):
        m = (m * np.where(bits[:, :, k] != 0, f32(-1.0), f32(1.0))).astype(f32)
        s = (f32(2.0) * s + m).astype(f32)
    return (s * pn).astype(f32)


def demodulate_scale(y, n, b, gain):
    """y: F x S float32 received symbols -> F x n float32 decoder inputs."""
    F, S = y.shape
    nm, _ = constants(b)
    out = np.empty((F, S, b), f32)
    a = (y.astype(f32) * nm).astype(f32)
    shift = f32(1 << (b - 1))
    for k in range(b):
        out[:, :, k] = a
        a = (np.abs(a) - shift).astype(f32)
        shift = f32(shift * f32(0.5))
    out = (out * f32(gain)).astype(f32)
    return np.ascontiguousarray(out.reshape(F, S * b)[:, :n])
