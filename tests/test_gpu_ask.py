"""pcg_ask_channel_f32 on the GPU: ASK modulate / AWGN or Rayleigh / demodulate / scale.

The deterministic stages are pinned bit for bit against the numpy model (tests/ask_numpy.py), the
noise against the existing BPSK-AWGN kernel (same Philox counters) and by its statistics."""
import numpy as np
import pytest

import ask_numpy

pytestmark = pytest.mark.gpu

SHAPES = [(8, 3), (16, 10), (16, 16), (1024, 1), (1024, 2), (1024, 3), (1024, 7), (1024, 10)]
FRAMES = [1, 3, 257]


def u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


_codes = {}


def codes(F, n):
    """Random packed code bits, the same for every test that asks for (F, n)."""
    if (F, n) not in _codes:
        c = np.random.default_rng(1000 * n + F).integers(0, 256, (F, n // 8), dtype=np.uint8)
        c.setflags(write=False)
        _codes[(F, n)] = c
    return _codes[(F, n)]


def channel(code, n, b, sigma, gain, seed, fading="awgn", want_symbols=True):
    import torch
    from antpolarcodes_amd._native import ask_channel_device
    dev = torch.device("cuda:0")
    F = code.shape[0]
    S = ask_numpy.symbol_count(n, b)
    d_code = torch.from_numpy(np.array(code)).to(dev)
    # guard rows either side: the kernel must write F x n and F x S floats and nothing else
    out = torch.full((F + 2, n), 7.25, dtype=torch.float32, device=dev)
    sym = torch.full((F + 2, S), 7.25, dtype=torch.float32, device=dev)
    ask_channel_device(d_code, n, b, sigma, gain, seed, out[1:F + 1], sym[1:F + 1] if want_symbols else None,
                       fading=fading)
    torch.cuda.synchronize()
    out, sym = out.cpu().numpy(), sym.cpu().numpy()
    assert (out[[0, -1]] == 7.25).all() and (sym[[0, -1]] == 7.25).all()
    if not want_symbols:
        assert (sym == 7.25).all()
    return out[1:-1], sym[1:-1]


@pytest.mark.parametrize("F", FRAMES)
@pytest.mark.parametrize("n,b", SHAPES)
def test_noiseless_stages_equal_numpy(n, b, F):
    code = codes(F, n)
    gain = 1.75
    out, sym = channel(code, n, b, 0.0, gain, seed=3)
    x = ask_numpy.modulate(code, n, b)
    assert np.array_equal(u32(sym), u32(x))
    assert np.array_equal(u32(out), u32(ask_numpy.demodulate_scale(x, n, b, gain)))
    out2, _ = channel(code, n, b, 0.0, gain, seed=3, want_symbols=False)
    assert np.array_equal(u32(out2), u32(out))


@pytest.mark.parametrize("fading", ["awgn", "rayleigh"])
@pytest.mark.parametrize("F", FRAMES)
@pytest.mark.parametrize("n,b", SHAPES)
def test_noisy_output_is_numpy_demodulation_of_the_returned_symbols(n, b, F, fading):
    code = codes(F, n)
    gain = 3.5
    out, sym = channel(code, n, b, 0.4, gain, seed=11, fading=fading)
    assert np.isfinite(sym).all()
    assert not np.array_equal(sym, ask_numpy.modulate(code, n, b))
    assert np.array_equal(u32(out), u32(ask_numpy.demodulate_scale(sym, n, b, gain)))


@pytest.mark.parametrize("F,n", [(257, 1024), (3, 8)])
def test_bpsk_awgn_symbols_equal_the_existing_kernel(F, n):
    import torch
    from antpolarcodes_amd._native import bpsk_awgn_device
    code = codes(F, n)
    sigma, seed = np.float32(0.7), 0x1234567890ABCDEF
    _, sym = channel(code, n, 1, float(sigma), 1.0, seed)
    dev = torch.device("cuda:0")
    llr = torch.empty((F, n), dtype=torch.float32, device=dev)
    bpsk_awgn_device(torch.from_numpy(np.array(code)).to(dev), n, float(sigma), seed, llr)
    torch.cuda.synchronize()
    scale = np.float32(np.float32(2.0) / np.float32(sigma * sigma))
    assert np.array_equal(u32((sym * scale).astype(np.float32)), u32(llr.cpu().numpy()))


@pytest.mark.parametrize("fading", ["awgn", "rayleigh"])
@pytest.mark.parametrize("n,b", [(1024, 1), (1024, 3), (1024, 10), (8, 3)])
def test_frame_noise_does_not_depend_on_the_launch_geometry(n, b, fading):
    code = codes(257, n)
    big, bsym = channel(code, n, b, 0.4, 2.0, seed=5, fading=fading)
    for F in (1, 3, 67):  # other grid sizes, the same leading frames
        small, ssym = channel(code[:F], n, b, 0.4, 2.0, seed=5, fading=fading)
        assert np.array_equal(u32(small), u32(big[:F]))
        assert np.array_equal(u32(ssym), u32(bsym[:F]))


@pytest.mark.parametrize("fading", ["awgn", "rayleigh"])
def test_seed_and_frame_select_the_noise(fading):
    n, b, F = 1024, 2, 3
    code = np.zeros((F, n // 8), np.uint8)  # equal rows: any difference is the noise
    a, asym = channel(code, n, b, 0.4, 1.0, seed=5, fading=fading)
    again, _ = channel(code, n, b, 0.4, 1.0, seed=5, fading=fading)
    assert a.tobytes() == again.tobytes()
    other, osym = channel(code, n, b, 0.4, 1.0, seed=6, fading=fading)
    assert (asym != osym).mean() > 0.99
    assert (asym[0] != asym[1]).mean() > 0.99 and (asym[1] != asym[2]).mean() > 0.99
    assert (asym[0, 1:] != asym[0, :-1]).mean() > 0.99  # and neighbouring symbols differ


# ---- statistics over M = 2^20 symbols (F = 1024, n = 1024, b = 1); bounds are 6 standard errors
M = 1 << 20
SIGMA = 0.5


@pytest.fixture(scope="module")
def stat_runs():
    code = codes(1024, 1024)
    x = ask_numpy.modulate(code, 1024, 1).astype(np.float64)
    runs = {"x": x}
    runs["awgn"] = channel(code, 1024, 1, SIGMA, 1.0, seed=77)[1].astype(np.float64)
    runs["fade"] = channel(code, 1024, 1, 0.0, 1.0, seed=77, fading="rayleigh")[1].astype(np.float64)
    runs["rayleigh"] = channel(code, 1024, 1, SIGMA, 1.0, seed=77, fading="rayleigh")[1].astype(np.float64)
    return runs


def test_awgn_noise_moments(stat_runs):
    g = ((stat_runs["awgn"] - stat_runs["x"]) / SIGMA).ravel()
    assert g.size == M
    mean, var = g.mean(), g.var()
    kurt = ((g - mean) ** 4).mean() / var ** 2 - 3.0
    print(f"awgn noise: mean {mean:.3e} var-1 {var - 1:.3e} excess kurtosis {kurt:.3e}")
    assert abs(mean) < 6 * np.sqrt(1.0 / M)        # se of the mean of a unit normal
    assert abs(var - 1.0) < 6 * np.sqrt(2.0 / M)   # se of the variance
    assert abs(kurt) < 6 * np.sqrt(24.0 / M)       # se of the excess kurtosis


def test_rayleigh_fading_moments(stat_runs):
    h = (stat_runs["fade"] / stat_runs["x"]).ravel()
    assert (h >= 0).all()
    # h = sqrt(g1^2 + g2^2): E h = sqrt(pi/2), E h^2 = 2, Var h = 2 - pi/2, Var h^2 = 4 (chi-square, 2 dof)
    m1, m2 = h.mean(), (h * h).mean()
    print(f"rayleigh: E[h]-sqrt(pi/2) {m1 - np.sqrt(np.pi / 2):.3e} E[h^2]-2 {m2 - 2:.3e}")
    assert abs(m1 - np.sqrt(np.pi / 2)) < 6 * np.sqrt((2 - np.pi / 2) / M)
    assert abs(m2 - 2.0) < 6 * np.sqrt(4.0 / M)


def test_rayleigh_noise_is_uncorrelated_with_the_fading(stat_runs):
    h = (stat_runs["fade"] / stat_runs["x"]).ravel()
    g = ((stat_runs["rayleigh"] - stat_runs["fade"]) / SIGMA).ravel()
    r =np.corrcoef(h, g)[0, 1]
    print(f"rayleigh: corr(h, noise) {r:.3e}")
    assert abs(r) < 6 / np.sqrt(M)  # se of a sample correlation of independent variables
