"""Each kernel of csrc/fs2_griffin_lim.hip alone against the fp64 restatement of its contract (tests/gl_ref.py), called through
_lib.call on the inputs of tests/gl_cases.py, at STFT sizes other than the production one.  Every input is NaN wherever the contract
says "never read" (padding rows and columns, rows past an utterance's frames), every output holds a sentinel first and must keep it
wherever the contract says "never written", and every leading dimension is larger than it has to be unless the case is about the
tight one.  Elementwise bars are tests/golden/gl_kernel_bars.json (4 x the oracle's own float32-to-fp64 distance, normalised as
tests/gl_cases.py states); whatever holds a GEMM is held to the forward-error bound (K + 2) 2^-24 sum |x| |w| of a K-term sum in any
order (K roundings of the sum and products, 2 for the float32 casts of the stored basis), evaluated per element in fp64, with the
elementwise bars carried through the linear steps after it.  Every test prints its largest error / bar.

    entry point           called directly by
    fs2_gl_mag_phase      test_mag_phase, test_project_equals_mag_phase_then_recombine, test_rows_above_65535
    fs2_gl_recombine      test_recombine, test_project_equals_mag_phase_then_recombine, test_rows_above_65535
    fs2_gl_project        test_project, test_project_equals_mag_phase_then_recombine, test_rows_above_65535
    fs2_gl_ola            test_ola, test_ola_envelope_is_window_sumsquare_bit_for_bit, test_ola_rows_are_independent
    fs2_gl_mel_to_mag     test_mel_to_mag
    (all five)            test_refusals, test_direct_calls_are_deterministic
    (STFT / griffin_lim)  test_one_iteration_is_the_chain_of_its_parts, test_transform_inverse_griffin_lim_at_other_sizes
"""
import numpy as np
import pytest
import torch

from fastspeech2_amd import _lib, ops
from tests import gl_cases as C
from tests import gl_ref

pytestmark = pytest.mark.gpu
NAN = np.float32("nan")
SENT = np.float32(-7777.25)                          # what every output holds before a call
U = 2.0 ** -24


@pytest.fixture(scope="module")
def bars():
    return C.bars()


def _d(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _frames_d(frames, dev):
    """frames followed by a poisoned entry the kernels must not read"""
    return None if frames is None else _d(np.asarray(list(frames) + [1 << 30], np.int32), dev)


def _nframes(frames, B, Fmax):
    return [Fmax] * B if frames is None else [min(max(f, 0), Fmax) for f in frames]


def _kept(a):
    return a.size == 0 or bool(np.all(a == SENT))


def _held(name, got, ref, unit, bar):
    """|got - ref| <= bar * unit wherever unit > 0, got == 0 exactly wherever unit == 0 (there ref is 0) -> largest error / bar"""
    got, ref, unit = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.asarray(unit, np.float64)
    assert got.shape == ref.shape == unit.shape, (name, got.shape, ref.shape, unit.shape)
    zero = unit == 0
    assert not ref[zero].any() and not got[zero].any(), (name, "non-zero where the contract says 0", np.argwhere(zero & (got != 0))[:4])
    r = np.abs(got - ref)[~zero] / unit[~zero]
    worst = float(r.max()) / bar if r.size else 0.0
    assert np.isfinite(got).all() and worst <= 1.0, (name, "largest error / bar", worst, "bar", bar)
    return worst


def _strided(vals, layout, frames, dev):
    """vals (B, Fmax, NF) as a view of a larger NaN buffer, NaN in the rows past frames -> (tensor, sb, sf, sk).
    'frame': (B, Fmax, NF) as the loop passes it; 'channel': (B, NF, Fmax) as STFT.inverse passes it."""
    B, Fmax, NF = vals.shape
    v = vals.copy()
    for b, F in enumerate(_nframes(frames, B, Fmax)):
        v[b, F:] = NAN
    if layout == "frame":
        buf = np.full((B, Fmax + 1, NF + 2), NAN, np.float32)
        buf[:, :Fmax, :NF] = v
        return _d(buf, dev), (Fmax + 1) * (NF + 2), NF + 2, 1
    buf = np.full((B, NF + 1, Fmax + 2), NAN, np.float32)
    buf[:, :NF, :Fmax] = v.transpose(0, 2, 1)
    return _d(buf, dev), (NF + 1) * (Fmax + 2), 1, Fmax + 2


def _ft_rows(vals, frames, Fmax, pad, dev):
    """vals (B, S, 2 NF) -> (B * S, 2 NF + pad) device rows, NaN in the padding columns and in every row f >= frames[b]"""
    B, S, W = vals.shape
    buf = np.full((B, S, W + pad), NAN, np.float32)
    for b, F in enumerate(_nframes(frames, B, Fmax)):
        buf[b, :F, :W] = vals[b, :F]
    return _d(buf.reshape(B * S, W + pad), dev)


# ---------------------------------------------------------------------------------------------- direct calls
def call_mag_phase(dev, vals, pad=3, extra_rows=2):
    B, F, W = vals.shape
    NF, S = W // 2, F + extra_rows
    ft = _ft_rows(np.concatenate([vals, np.zeros((B, extra_rows, W), np.float32)], axis=1), None, F, pad, dev)
    mag = torch.full((B * NF * F + 5,), float(SENT), device=dev)
    phase = torch.full((B * NF * F + 5,), float(SENT), device=dev)
    _lib.call("fs2_gl_mag_phase", ft.data_ptr(), ft.stride(0), S, mag.data_ptr(), phase.data_ptr(), B, F, NF, ops._stream())
    mag, phase = mag.cpu().numpy(), phase.cpu().numpy()
    assert _kept(mag[B * NF * F:]) and _kept(phase[B * NF * F:])
    return mag[:B * NF * F].reshape(B, NF, F), phase[:B * NF * F].reshape(B, NF, F)


def call_recombine(dev, mag, ph, frames, ldg, layout, ph_layout=None):
    B, Fmax, NF = mag.shape
    m, msb, msf, msk = _strided(mag, layout, frames, dev)
    p, psb, psf, psk = _strided(ph, ph_layout or layout, frames, dev)
    fr = _frames_d(frames, dev)
    G = torch.full((B * Fmax + 1, ldg), float(SENT), device=dev)
    _lib.call("fs2_gl_recombine", m.data_ptr(), msb, msf, msk, p.data_ptr(), psb, psf, psk, ops._p(fr), G.data_ptr(), ldg, B, Fmax, NF,
              ops._stream())
    G = G.cpu().numpy()
    assert _kept(G[B * Fmax])
    return G[:B * Fmax].reshape(B, Fmax, ldg)


def call_project(dev, ftv, mag, frames, ldg, layout, pad=5):
    B, Fmax, NF = mag.shape
    S = ftv.shape[1]
    ft = _ft_rows(ftv, frames, Fmax, pad, dev)
    m, msb, msf, msk = _strided(mag, layout, frames, dev)
    fr = _frames_d(frames, dev)
    G = torch.full((B * Fmax + 1, ldg), float(SENT), device=dev)
    _lib.call("fs2_gl_project", ft.data_ptr(), ft.stride(0), S, m.data_ptr(), msb, msf, msk, ops._p(fr), G.data_ptr(), ldg, B, Fmax, NF,
              ops._stream())
    G = G.cpu().numpy()
    assert _kept(G[B * Fmax])
    return G[:B * Fmax].reshape(B, Fmax, ldg)


def call_ola(dev, c, filt, hop, form="both", only_row=None, seg=None, win_sq=None):
    """form: 'xp', 'y' or 'both'.  only_row: every other utterance's segments are NaN."""
    seg = c["seg"] if seg is None else seg
    B, Fmax = seg.shape[:2]
    buf = np.full((B, Fmax, c["lds"]), NAN, np.float32)
    for b, F in enumerate(_nframes(c["frames"], B, Fmax)):
        if only_row is None or b == only_row:
            buf[b, :F, :filt] = seg[b, :F]
    s = _d(buf.reshape(B * Fmax, c["lds"]), dev)
    fr = _frames_d(c["frames"], dev)
    w2 = _d(np.concatenate([np.asarray(c["win_sq"] if win_sq is None else win_sq, np.float64), [np.nan] * 3]), dev)
    xp = torch.full((B + 1, c["row_len"]), float(SENT), device=dev)
    y = torch.full((B + 1, c["ldy"]), float(SENT), device=dev)
    _lib.call("fs2_gl_ola", s.data_ptr(), c["lds"], ops._p(fr), w2.data_ptr(), xp.data_ptr() if form != "y" else None, c["row_len"],
              y.data_ptr() if form != "xp" else None, c["ldy"], B, Fmax, filt, hop, ops._stream())
    xp, y = xp.cpu().numpy(), y.cpu().numpy()
    assert _kept(xp[B]) and _kept(y[B])
    assert form != "y" or _kept(xp)
    assert form != "xp" or _kept(y)
    return xp[:B], y[:B]


def call_mel_to_mag(dev, mel, lens, basis, span, pad=3):
    """mel (B, n_mel, T) as a non-contiguous view ((b, j, t) at b*sb + t*(n_mel + 2) + j), NaN from each utterance's last frame on"""
    B, n_mel, T = mel.shape
    NF, Fmax, ldm = basis.shape[1], T - 1, basis.shape[1] + pad
    buf = np.full((B, T + 1, n_mel + 2), NAN, np.float32)
    for b, n in enumerate(lens):
        buf[b, :max(n - 1, 0), :n_mel] = mel[b, :, :max(n - 1, 0)].T
    m = _d(buf, dev)
    ln = _d(np.asarray(list(lens) + [1 << 30], np.int32), dev)
    mag = torch.full((B * Fmax + 1, ldm), float(SENT), device=dev)
    bs, sp = _d(basis, dev), _d(span, dev)
    _lib.call("fs2_gl_mel_to_mag", m.data_ptr(), (T + 1) * (n_mel + 2), 1, n_mel + 2, ln.data_ptr(), bs.data_ptr(), sp.data_ptr(),
              mag.data_ptr(), ldm, B, Fmax, n_mel, NF, ops._stream())
    mag = mag.cpu().numpy()
    assert _kept(mag[B * Fmax]) and _kept(mag[:, NF:])
    return mag[:B * Fmax, :NF].reshape(B, Fmax, NF)


# ---------------------------------------------------------------------------------------------- fs2_gl_mag_phase
@pytest.mark.parametrize("NF", [C.nf_of(f) for f, _ in C.SIZES])
def test_mag_phase(dev, bars, NF):
    ft = C.mag_phase_case(NF)
    mag, phase = call_mag_phase(dev, ft)
    m64, p64 = gl_ref.mag_phase(ft)
    wm = _held("mag", mag, m64, m64, bars["mag_rel"][str(NF)])
    wp = _held("phase", phase, p64, np.ones_like(p64), bars["phase"][str(NF)])
    re, im = ft[..., :NF], ft[..., NF:]
    m32 = np.sqrt(re * re + im * im).transpose(0, 2, 1)                      # float32: each product and the sum rounded
    ulps = np.abs(mag.view(np.int32).astype(np.int64) - m32.view(np.int32).astype(np.int64))
    assert ulps.max() <= 1, ulps.max()
    print(f"mag_phase NF {NF}: mag error / bar {wm:.3f}, phase error / bar {wp:.3f}, {int((ulps != 0).sum())} of {ulps.size} magnitudes "
          f"differ from numpy's float32 sqrt(re*re + im*im) (by 1 ulp)")
    for b, f in ((0, 0), (ft.shape[0] - 1, ft.shape[1] - 1)):
        assert mag[b, 0, f] == 0 and phase[b, 0, f] == 0 and not np.signbit(phase[b, 0, f])          # (0, 0)
        assert phase[b, 1, f] > 3 and phase[b, 2, f] < -3                                            # (-x, +0) -> +pi, (-x, -0) -> -pi
        assert mag[b, 1, f] == mag[b, 2, f] == np.float32(3.5)
        assert mag[b, 3, f] == mag[b, 4, f] == np.float32(2.25) and phase[b, 3, f] > 0 > phase[b, 4, f]   # pure imaginary


# ---------------------------------------------------------------------------------------------- fs2_gl_recombine
def _unit(mag, frames, ldg):
    """[m | m | 0 ...] per row, 0 in the rows past frames: what the error of G is measured per unit of"""
    B, Fmax, NF = mag.shape
    u = np.zeros((B, Fmax, ldg))
    for b, F in enumerate(_nframes(frames, B, Fmax)):
        u[b, :F, :NF] = u[b, :F, NF:2 * NF] = mag[b, :F]
    return u


@pytest.mark.parametrize("layout", ["channel", "frame"])
@pytest.mark.parametrize("NF", [C.nf_of(f) for f, _ in C.SIZES])
def test_recombine(dev, bars, NF, layout):
    mag, ph = C.mag_case(NF), C.phase_case(NF)
    worst = 0.0
    for frames in (None, C.FRAMES):
        for ldg in (2 * NF, 2 * NF + 2, 2 * NF + 6):
            G = call_recombine(dev, mag, ph, frames, ldg, layout)
            worst = max(worst, _held(f"recombine {frames} {ldg}", G, gl_ref.recombine(mag, ph, frames, ldg), _unit(mag, frames, ldg),
                                     bars["recombine"][str(NF)]))
            # phase 0: cos = 1, sin = 0 exactly
            assert np.array_equal(G[2:4, 0, 4], mag[2:4, 0, 4]) and not G[2:4, 0, NF + 4].any()
    print(f"recombine NF {NF} {layout}-major: largest error / bar {worst:.3f}")


# ---------------------------------------------------------------------------------------------- fs2_gl_project
@pytest.mark.parametrize("NF", [C.nf_of(f) for f, _ in C.SIZES])
def test_project(dev, bars, NF):
    mag, ftv = C.mag_case(NF), C.ft_case(NF)
    worst = 0.0
    for frames in (None, C.FRAMES):
        for ldg in (2 * NF, 2 * NF + 2, 2 * NF + 6):
            G = call_project(dev, ftv, mag, frames, ldg, "frame" if ldg != 2 * NF + 2 else "channel")
            worst = max(worst, _held(f"project {frames} {ldg}", G, gl_ref.project(ftv, mag, frames, ldg), _unit(mag, frames, ldg),
                                     bars["project"][str(NF)]))
            assert np.array_equal(G[2:4, 0, 0], mag[2:4, 0, 0]) and not G[2:4, 0, NF].any()          # (0, 0) -> phase 0 -> (m, 0)
    print(f"project NF {NF}: largest error / bar {worst:.3f}")


@pytest.mark.parametrize("NF", [C.nf_of(f) for f, _ in C.SIZES])
def test_project_equals_mag_phase_then_recombine(dev, NF):
    """project evaluates m cos(atan2(im, re)), m sin(atan2(im, re)): the expressions mag_phase and recombine evaluate on the same
    float32 values, so the two routes agree bit for bit"""
    mag, ftv = C.mag_case(NF), C.ft_case(NF)
    Fmax = mag.shape[1]
    _, phase = call_mag_phase(dev, ftv[:, :Fmax])                                         # (B, NF, Fmax)
    for frames in (None, C.FRAMES):
        G = call_project(dev, ftv, mag, frames, 2 * NF + 2, "frame")
        G2 = call_recombine(dev, mag, np.ascontiguousarray(phase.transpose(0, 2, 1)), frames, 2 * NF + 2, "frame", ph_layout="channel")
        assert np.array_equal(G, G2), (frames, int((G != G2).sum()), float(np.abs(G - G2).max()))


# ---------------------------------------------------------------------------------------------- fs2_gl_ola
@pytest.mark.parametrize("setting", C.OLA_SETTINGS, ids=lambda s: "-".join(map(str, s)))
def test_ola(dev, bars, setting):
    filt, hop, win = setting
    c = C.ola_case(filt, hop, win)
    (xp64, y64), (uxp, uy) = C.ola_ref(c, filt, hop), C.ola_ref(c, filt, hop, absolute=True)
    bar = bars["ola"][f"{filt},{hop},{win}"]
    P, worst, both = filt // 2, 0.0, None
    for form in ("both", "xp", "y"):
        xp, y = call_ola(dev, c, filt, hop, form)
        if form != "y":
            worst = max(worst, _held(f"ola xp {form}", xp, xp64, uxp, bar))
        if form != "xp":
            worst = max(worst, _held(f"ola y {form}", y, y64, uy, bar))
        if form == "both":
            both = (xp, y)
        else:                                                            # the two outputs do not depend on each other being asked for
            assert form == "y" or np.array_equal(xp, both[0])
            assert form == "xp" or np.array_equal(y, both[1])
    xp, y = both
    for b, F in enumerate(_nframes(c["frames"], len(c["frames"]), c["Fmax"])):
        N = hop * (F - 1)
        assert not y[b, max(N, 0):].any()
        if N <= P:
            assert not xp[b].any(), (b, F)
        else:                                                            # xp is y reflected at the utterance's own end, bit for bit
            assert np.array_equal(xp[b, :N + filt], np.pad(y[b, :N], (P, P), mode="reflect")) and not xp[b, N + filt:].any(), (b, F)
    if win < filt:
        assert (gl_ref.window_sumsquare(c["Fmax"], hop, win, filt) == 0).any()          # the env > tiny branch is taken both ways
    print(f"ola {setting}: largest error / bar {worst:.3f}")


@pytest.mark.parametrize("setting", C.OLA_SETTINGS[:-1], ids=lambda s: "-".join(map(str, s)))
def test_ola_envelope_is_window_sumsquare_bit_for_bit(dev, setting):
    """segments of ones: the overlap-add is the count of covering frames, so the output is count / envelope * (filt / hop) in
    float32 with the envelope audio.window_sumsquare builds (numpy: a float32 array += float64 window^2, frame by frame)"""
    from fastspeech2_amd.audio import _window, window_sumsquare
    filt, hop, win = setting
    F = filt // hop + 5
    N, P = hop * (F - 1), filt // 2
    c = {"frames": [F, 2], "lds": filt, "row_len": N + filt, "ldy": N}
    _, y = call_ola(dev, c, filt, hop, "both", seg=np.ones((2, F, filt), np.float32), win_sq=_window("hann", win, filt) ** 2)
    for b, Fb in enumerate(c["frames"]):
        env = window_sumsquare("hann", Fb, hop, win, filt)
        count = np.zeros(env.size, np.float32)
        for f in range(Fb):
            count[f * hop:f * hop + filt] += 1
        nz = env > gl_ref.TINY32
        want = count.copy()
        want[nz] = count[nz] / env[nz]
        want = (want * np.float32(filt / hop))[P:P + hop * (Fb - 1)]
        assert want.dtype == np.float32 and np.array_equal(y[b, :want.size], want), (b, int((y[b, :want.size] != want).sum()))
        assert win == filt or not nz.all()


@pytest.mark.parametrize("setting", [(1024, 256, 256), (256, 64, 200), (24, 10, 24)], ids=lambda s: "-".join(map(str, s)))
def test_ola_rows_are_independent(dev, setting):
    filt, hop, win = setting
    c = C.ola_case(filt, hop, win)
    xp, y = call_ola(dev, c, filt, hop)
    for b in range(len(c["frames"])):
        xb, yb = call_ola(dev, c, filt, hop, only_row=b)
        assert np.array_equal(xb[b], xp[b]) and np.array_equal(yb[b], y[b]), b


# ---------------------------------------------------------------------------------------------- fs2_gl_mel_to_mag
@pytest.mark.parametrize("n_mel,NF,T", [(256, 129, 6), (7, 9, 5)])
def test_mel_to_mag(dev, n_mel, NF, T):
    mel, lens, basis, span = C.mel_case(n_mel, NF, T)
    got = call_mel_to_mag(dev, mel, lens, basis, span)
    ref, bound = C.mel_ref(mel, lens, basis, span)
    k = np.arange(NF)
    uncovered = ~((k[None, :] >= span[:, :1]) & (k[None, :] < span[:, 1:])).any(0)
    assert uncovered[0] and uncovered[-2:].all() and not got[..., uncovered].any()
    assert not got[0].any() and not got[1].any() and not got[2, 1:].any() and got[2, 0].any() and got[3].any()
    worst = _held("mel_to_mag", got, ref, bound, 1.0)
    print(f"mel_to_mag n_mel {n_mel} NF {NF}: largest error / bound {worst:.3f}")


# ---------------------------------------------------------------------------------------------- refusals
def test_refusals(dev):
    """every FS2_CHECK_ARG line of the five entry points raises ValueError, leaves its outputs alone, and the next call is judged afresh"""
    st = ops._stream()
    f = torch.full((4096,), float(SENT), device=dev)
    i = torch.ones(8, dtype=torch.int32, device=dev)
    d = torch.ones(64, dtype=torch.float64, device=dev)
    p, ip, dp = f.data_ptr(), i.data_ptr(), d.data_ptr()
    bad = [
        ("fs2_gl_mel_to_mag", (p, 64, 1, 8, ip, p, ip, None, 9, 1, 4, 8, 9, st)),                  # null
        ("fs2_gl_mel_to_mag", (p, 64, 1, 8, ip, p, ip, p, 9, 1, 4, 257, 9, st)),                   # n_mel = 257
        ("fs2_gl_mel_to_mag", (p, 64, 1, 8, ip, p, ip, p, 8, 1, 4, 8, 9, st)),                     # ldm < NF
        ("fs2_gl_mel_to_mag", (p, 64, 1, 8, ip, p, ip, p, 9, 1, 0, 8, 9, st)),                     # Fmax = 0
        ("fs2_gl_recombine", (p, 36, 9, 1, p, 36, 9, 1, ip, None, 18, 1, 4, 9, st)),               # null
        ("fs2_gl_recombine", (p, 36, 9, 1, p, 36, 9, 1, ip, p, 17, 1, 4, 9, st)),                  # ldg < 2 NF
        ("fs2_gl_recombine", (p, 36, 9, 1, p, 36, 9, 1, ip, p, 18, 1, 0, 9, st)),                  # Fmax = 0
        ("fs2_gl_project", (None, 18, 6, p, 36, 9, 1, ip, p, 18, 1, 4, 9, st)),                    # null
        ("fs2_gl_project", (p, 18, 3, p, 36, 9, 1, ip, p, 18, 1, 4, 9, st)),                       # S < Fmax
        ("fs2_gl_project", (p, 17, 6, p, 36, 9, 1, ip, p, 18, 1, 4, 9, st)),                       # ldft < 2 NF
        ("fs2_gl_project", (p, 18, 6, p, 36, 9, 1, ip, p, 17, 1, 4, 9, st)),                       # ldg < 2 NF
        ("fs2_gl_ola", (p, 16, ip, dp, None, 64, None, 32, 1, 4, 16, 4, st)),                      # neither xp nor y
        ("fs2_gl_ola", (p, 16, ip, None, p, 64, p, 32, 1, 4, 16, 4, st)),                          # null window
        ("fs2_gl_ola", (p, 15, ip, dp, p, 64, p, 32, 1, 4, 16, 4, st)),                            # lds < filter
        ("fs2_gl_ola", (p, 16, ip, dp, p, 64, p, 32, 1, 4, 15, 5, st)),                            # odd filter
        ("fs2_gl_ola", (p, 16, ip, dp, p, 64, p, 32, 1, 4, 4, 8, st)),                             # filter < hop
        ("fs2_gl_ola", (p, 16, ip, dp, p, 64, p, 32, 1, 4, 16, 0, st)),                            # hop = 0
        ("fs2_gl_ola", (p, 16, ip, dp, p, 27, p, 32, 1, 4, 16, 4, st)),                            # xp rows < hop (Fmax - 1) + filter = 28
        ("fs2_gl_ola", (p, 16, ip, dp, p, 64, p, 11, 1, 4, 16, 4, st)),                            # y rows < hop (Fmax - 1) = 12
        ("fs2_gl_mag_phase", (p, 18, 6, None, p, 1, 4, 9, st)),                                    # null
        ("fs2_gl_mag_phase", (p, 18, 3, p, p, 1, 4, 9, st)),                                       # S < F
        ("fs2_gl_mag_phase", (p, 17, 6, p, p, 1, 4, 9, st)),                                       # ldft < 2 NF
        ("fs2_gl_mag_phase", (p, 18, 6, p, p, 1, 0, 9, st)),                                       # F = 0
        ("fs2_gl_mag_phase", (p, 18, 6, p, p, -1, 4, 9, st)),                                      # B < 0
    ]
    for name, args in bad:
        with pytest.raises(ValueError):
            _lib.call(name, *args)
    torch.cuda.synchronize()
    assert _kept(f.cpu().numpy())


# ---------------------------------------------------------------------------------------------- determinism
def test_direct_calls_are_deterministic(dev):
    NF = 129
    mag, ph, ftv = C.mag_case(NF), C.phase_case(NF), C.ft_case(NF)
    c = C.ola_case(256, 64, 200)
    mel = C.mel_case(256, 129, 6)
    calls = {
        "mag_phase": lambda: call_mag_phase(dev, C.mag_phase_case(NF)),
        "recombine": lambda: (call_recombine(dev, mag, ph, C.FRAMES, 2 * NF + 6, "channel"),),
        "project": lambda: (call_project(dev, ftv, mag, C.FRAMES, 2 * NF + 6, "frame"),),
        "ola": lambda: call_ola(dev, c, 256, 64),
        "mel_to_mag": lambda: (call_mel_to_mag(dev, *mel),),
    }
    for name, fn in calls.items():
        a, b = fn(), fn()
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)), name


# ---------------------------------------------------------------------------------------------- the iteration as a chain
def test_one_iteration_is_the_chain_of_its_parts(dev):
    """griffin_lim_rows(n_iters=1) on a ragged batch = per utterance inverse -> transform -> inverse of the utterance alone, bit for
    bit: the loop's xp (fs2_gl_ola) against fs2_reflect_pad of the signal, its project against mag_phase -> recombine"""
    from fastspeech2_amd.audio import STFT
    filt, hop, NF = 256, 64, 129
    stft = STFT(filt, hop, 256).to(dev)
    frames, Fmax = [5, 9, 6], 9
    rng = np.random.RandomState(4)
    mag = np.exp(rng.standard_normal((3, Fmax, NF))).astype(np.float32)
    ang = rng.uniform(-np.pi, np.pi, (3, NF, Fmax)).astype(np.float32)
    m, msb, msf, msk = _strided(mag, "frame", frames, dev)
    a = _d(ang, dev)
    y = stft.griffin_lim_rows(m, (msb, msf, msk, Fmax), _d(np.asarray(frames, np.int32), dev), a, (a.stride(0), a.stride(2), a.stride(1)), 1)
    y = y.cpu().numpy()
    for b, F in enumerate(frames):
        mb = _d(mag[b:b + 1, :F].transpose(0, 2, 1), dev)
        y0 = stft.inverse(mb, _d(ang[b:b + 1, :, :F], dev))
        _, ph = stft.transform(y0[:, 0].clone())
        y1 = stft.inverse(mb, ph).cpu().numpy()[0, 0]
        N = hop * (F - 1)
        assert y1.shape == (N,) and np.isfinite(y1).all() and np.array_equal(y[b, :N], y1), (b, int((y[b, :N] != y1).sum()))
        assert not y[b, N:].any()


# ---------------------------------------------------------------------------------------------- whole transform / inverse / griffin_lim
def _signal(kind, N, seed):
    t = np.arange(N)
    if kind == "sines":
        x = 0.5 * np.sin(2 * np.pi * 0.031 * t) + 0.3 * np.sin(2 * np.pi * 0.117 * t + 1.0) + 0.1 * np.sin(2 * np.pi * 0.37 * t + 2.0)
    else:
        x = 0.3 * np.random.RandomState(seed).standard_normal(N)
    return x.astype(np.float32)[None]


@pytest.mark.parametrize("setting", [(256, 64, 256), (512, 128, 400), (1024, 256, 256), (64, 64, 64)], ids=lambda s: "-".join(map(str, s)))
def test_transform_inverse_griffin_lim_at_other_sizes(dev, bars, setting):
    from fastspeech2_amd.audio import STFT, griffin_lim
    filt, hop, win = setting
    NF = filt // 2 + 1
    stft, ref = STFT(filt, hop, win).to(dev), gl_ref.STFT(filt, hop, win)
    # relative elementwise bars do not depend on the size: the largest recorded one of each kind
    e_mag, e_ph, e_rec, e_ola = (max(bars[k].values()) for k in ("mag_rel", "phase", "recombine", "ola"))
    w2 = gl_ref.window(win, filt) ** 2
    for kind, F in (("sines", 12), ("noise", 37)):
        N = hop * (F - 1)
        x = _signal(kind, N, filt + F)
        # transform: ft = frames . basis^T over K = filt terms, then mag = |ft| (1-Lipschitz) and phase = arg ft (a disc of radius
        # r around ft subtends asin(r / |ft|))
        mag, phase = (t.cpu().numpy() for t in stft.transform(_d(x, dev)))
        m64, p64 = ref.transform(x)
        assert mag.shape == m64.shape == (1, NF, F)
        e_ft = (filt + 2) * U * (np.abs(ref.frames_of(x)) @ np.abs(ref.forward_basis.T))                 # (1, F, 2 NF)
        r = np.hypot(e_ft[..., :NF], e_ft[..., NF:]).transpose(0, 2, 1)
        w_mag = _held("transform mag", mag, m64, r + e_mag * m64, 1.0)
        keep = m64 > 1e-3 * m64.max()
        assert (r[keep] < m64[keep]).all()
        dph = gl_ref.phase_distance(phase, p64)[keep] / (np.arcsin(r[keep] / m64[keep]) + e_ph)
        assert dph.max() <= 1.0, ("transform phase", float(dph.max()))
        # inverse from (m64 as float32, seeded angles): G elementwise, seg = G . inverse_basis over K = 2 NF terms, overlap-add
        m32 = m64.astype(np.float32)
        ang = np.random.RandomState(F).uniform(-np.pi, np.pi, m32.shape).astype(np.float32)
        y = stft.inverse(_d(m32, dev), _d(ang, dev)).cpu().numpy()[:, 0]
        y64 = ref.inverse(m32, ang)
        G = gl_ref.recombine(m32.transpose(0, 2, 1), ang.transpose(0, 2, 1))
        mm = np.concatenate([m32, m32], axis=1).transpose(0, 2, 1).astype(np.float64)
        W = np.abs(ref.inverse_basis)
        e_seg = (2 * NF + 2) * U * (np.abs(G) @ W) + e_rec * (mm @ W)
        bound = gl_ref.ola(e_seg, None, w2, filt, hop, 0, N)[1] + e_ola * gl_ref.ola(np.abs(G @ ref.inverse_basis), None, w2, filt, hop, 0, N)[1]
        w_inv = _held("inverse", y, y64, bound, 1.0)
        y0 = griffin_lim(_d(m32, dev), stft, 0, angles=ang).cpu().numpy()
        w_gl0 = _held("griffin_lim 0", y0, y64, bound, 1.0)
        # one iteration: the projection is ill-conditioned at weak bins, so the signals are compared by their spectral convergence
        y1 = griffin_lim(_d(m32, dev), stft, 1, angles=ang).cpu().numpy()
        sc, sc64 = gl_ref.spectral_convergence(y1, m32, ref), gl_ref.spectral_convergence(gl_ref.griffin_lim(m32, ref, 1, ang), m32, ref)
        assert y1.shape == y64.shape and np.isfinite(y1).all() and abs(sc - sc64) <= 0.02 * sc64, (sc, sc64)
        print(f"{setting} {kind} F {F}: error / bound transform mag {w_mag:.4f} phase {float(dph.max()):.4f} inverse {w_inv:.4f} "
              f"griffin_lim(0) {w_gl0:.4f}; spectral convergence after 1 iteration {sc:.6f} (oracle {sc64:.6f})")


# ---------------------------------------------------------------------------------------------- more rows than grid y holds
def test_rows_above_65535(dev, bars):
    """65 540 rows of NF = 9 (a synthesis batch of 64 utterances of 1100 frames is 70 400): the row index is grid x, whose limit is
    2^31 - 1; grid y and z stop at 65 535"""
    mag, ph, ft, rows = C.big_case()
    R, NF = C.BIG_ROWS, C.BIG_NF
    ldg = 2 * NF + 2
    m, p, f = _d(mag, dev), _d(ph, dev), _d(ft, dev)
    fr = _d(np.asarray([R - 1], np.int32), dev)                                      # the last row is padding: zero
    unit = _unit(mag, [R - 1], ldg)[0, rows]
    st = ops._stream()
    G = torch.full((R + 1, ldg), float(SENT), device=dev)
    _lib.call("fs2_gl_recombine", m.data_ptr(), R * NF, NF, 1, p.data_ptr(), R * NF, NF, 1, fr.data_ptr(), G.data_ptr(), ldg, 1, R, NF, st)
    g = G.cpu().numpy()
    assert _kept(g[R])
    w_rec = _held("recombine", g[rows], gl_ref.recombine(mag[:, rows], ph[:, rows], None, ldg)[0] * (unit > 0), unit, bars["recombine"]["big"])
    G.fill_(float(SENT))
    _lib.call("fs2_gl_project", f.data_ptr(), 2 * NF, R, m.data_ptr(), R * NF, NF, 1, fr.data_ptr(), G.data_ptr(), ldg, 1, R, NF, st)
    g = G.cpu().numpy()
    assert _kept(g[R])
    w_pro = _held("project", g[rows], gl_ref.project(ft[:, rows], mag[:, rows], None, ldg)[0] * (unit > 0), unit, bars["project"]["big"])
    om = torch.full((NF * R + 3,), float(SENT), device=dev)
    op = torch.full((NF * R + 3,), float(SENT), device=dev)
    _lib.call("fs2_gl_mag_phase", f.data_ptr(), 2 * NF, R, om.data_ptr(), op.data_ptr(), 1, R, NF, st)
    om, op = om.cpu().numpy(), op.cpu().numpy()
    assert _kept(om[NF * R:]) and _kept(op[NF * R:]) and np.isfinite(om[:NF * R]).all() and np.isfinite(op[:NF * R]).all()
    m64, p64 = gl_ref.mag_phase(ft[:, rows])                                          # (1, NF, rows)
    w_mag = _held("mag", om[:NF * R].reshape(NF, R)[:, rows], m64[0], m64[0], bars["mag_rel"]["big"])
    w_ph = _held("phase", op[:NF * R].reshape(NF, R)[:, rows], p64[0], np.ones_like(p64[0]), bars["phase"]["big"])
    print(f"{R} rows: error / bar recombine {w_rec:.3f} project {w_pro:.3f} mag {w_mag:.3f} phase {w_ph:.3f}")
