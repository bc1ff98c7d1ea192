"""tests/stft_truth.py checked without a GPU: the float64 statement against a DFT written out, the case matrix against the properties
each case is there for, and the fp32 oracle's own error on every forward case (printed: it is the bar the GPU tests take)."""
import math

import pytest
import torch

import stft_truth as st
from conftest import report
from oracle import ref_cpu


def direct_mag(x, n_fft, win, hop):
    """O(N^2), every index written out: reflect by hand, window, sum over n of cos / sin at exactly reduced angles"""
    B, L = x.shape
    pad, T, K = (n_fft - hop) // 2, L // hop, n_fft // 2 + 1
    w = torch.zeros(n_fft, dtype=torch.float64)
    for n in range(win):
        w[(n_fft - win) // 2 + n] = float(torch.hann_window(win, dtype=torch.float32)[n])
    kn = (torch.arange(K)[:, None] * torch.arange(n_fft)[None, :]) % n_fft
    ang = 2.0 * math.pi * kn.double() / n_fft
    out = torch.zeros(B, T, K, dtype=torch.float64)
    for b in range(B):
        for t in range(T):
            fr = torch.zeros(n_fft, dtype=torch.float64)
            for n in range(n_fft):
                s = t * hop - pad + n
                if s < 0:
                    s = -s
                if s >= L:
                    s = 2 * (L - 1) - s
                assert 0 <= s < L
                fr[n] = float(x[b, s]) * w[n]
            re, im = (ang.cos() * fr).sum(1), -(ang.sin() * fr).sum(1)
            out[b, t] = torch.sqrt(re * re + im * im + 1e-9)
    return out


@pytest.mark.parametrize("L,hop,win", [(300, 128, 512), (700, 128, 512), (431, 50, 241)])
def test_truth_against_a_written_out_dft(L, hop, win):
    """a clip shorter than n_fft (one frame reflects at both ends), L % hop != 0, and an odd short window"""
    x = torch.randn(2, L, generator=torch.Generator().manual_seed(L)) * 0.3
    fr, norm = st.frames64(x, 512, win, hop)
    assert L % hop != 0 and fr.shape == (2, L // hop, 512) and norm.shape == (2, L // hop)
    want = direct_mag(x, 512, win, hop)
    got = st.mag64(fr)
    assert float(((got - want).abs() / (norm[..., None] + want)).max()) < 1e-13
    assert st.e_lin(want, got, norm) < 1e-5             # the same in the units of the GPU tests


@pytest.mark.parametrize("n_fft,hop,win,L", [(1024, 256, 1024, 2100), (2048, 240, 1200, 2500), (512, 512, 512, 1536), (512, 2, 512, 600)])
def test_truth_against_the_oracle_in_float64(n_fft, hop, win, L):
    x = (torch.randn(2, L, generator=torch.Generator().manual_seed(L)) * 0.3).double()
    fr, norm = st.frames64(x, n_fft, win, hop)
    want = ref_cpu.stft_magnitude(x, n_fft, win, hop).transpose(1, 2)
    # the oracle's float64 window is not the fp32 window cast up: hand it the same one
    spec = torch.stft(torch.nn.functional.pad(x[:, None], ((n_fft - hop) // 2,) * 2, mode="reflect")[:, 0] if n_fft != hop else x, n_fft,
                      hop_length=hop, win_length=win, window=torch.hann_window(win, dtype=torch.float32).double(), center=False,
                      return_complex=True)
    same_window = torch.sqrt(spec.real ** 2 + spec.imag ** 2 + 1e-9).transpose(1, 2)
    got = st.mag64(fr)
    assert got.shape == want.shape == (2, L // hop, n_fft // 2 + 1)
    assert float(((got - same_window).abs() / (norm[..., None] + same_window)).max()) < 1e-13
    # what the two windows differ by: every entry by at most 2^-25, so a bin by at most 2^-25 |frame|_1 <= 2^-25 sqrt(n_fft) |frame|_2,
    # and on noise the unwindowed frame has less than twice the norm of the Hann-windowed one
    assert float(((got - want).abs() / (norm[..., None] + want)).max()) < 2.0 ** -25 * math.sqrt(n_fft) * 2.0


def test_mel_truth_is_the_dense_product():
    basis = st.mel_basis(st.PROD_24K)
    mag = torch.rand(2, 5, 513, dtype=torch.float64)
    got = st.mel64(mag, basis)
    assert got.shape == (2, 100, 5)
    assert torch.allclose(got[1, :, 3], basis.double() @ mag[1, 3], rtol=1e-14, atol=0)


@pytest.mark.parametrize("name", list(st.MEL_EDGES))
def test_every_mel_table_has_the_property_it_is_there_for(name):
    mel, want = st.MEL_EDGES[name]
    p = st.mel_properties(st.mel_basis(mel))
    assert {k: p[k] for k in want} == want, p
    assert p["passes"] <= st.MAX_MEL_PASSES and p["chunks"] <= 64 * st.MAX_MEL_PASSES


def test_the_mel_edges_are_edges():
    p = {k: st.mel_properties(st.mel_basis(m)) for k, (m, _) in st.MEL_EDGES.items()}
    assert p["8k_2048_128"]["passes"] == st.MAX_MEL_PASSES                                   # the most the kernel holds
    assert p["48k_512_128"]["nyquist"] and p["44k_2048_128"]["nyquist"]                      # the last chunk reads the pad bins
    assert p["24k_512_1"]["widest"] == 255 and p["24k_512_1"]["chunks"] == 32                # one lane sums 32 chunks
    assert st.MEL_EDGES["24k_1024_64"][0].n_mels == 64 and st.MEL_EDGES["24k_1024_65"][0].n_mels == 65
    assert p["24k_1024_80_50_7600"]["top_bin"] < 512 * 2 // 3                                # a third of the bins feeds nothing
    # the basis of every band is one run of bins without a hole: first bin .. last bin is what the plan packs
    for k, (m, _) in st.MEL_EDGES.items():
        nz = st.mel_basis(m) != 0
        for row in nz:
            idx = torch.nonzero(row).flatten()
            assert idx.numel() == 0 or bool(row[idx[0]:idx[-1] + 1].all()), k


def test_every_case_is_a_legal_shape():
    ids = [c.id for c in st.FORWARD]
    assert len(set(ids)) == len(ids) and len({c.id for c in st.BACKWARD}) == len(st.BACKWARD)
    for c in st.FORWARD + st.BACKWARD:
        assert st.legal(c.n_fft, c.hop, c.L), c
        assert 0 < c.win <= c.n_fft
    for c in st.FORWARD:
        assert c.mel.n_fft == c.n_fft and c.L <= 65 * 512 + 511
    for n in (512, 1024, 2048):
        pad = (n - n // 4) // 2
        by_id = {c.id: c for c in st.GEOMETRY}
        assert by_id[f"{n}-smallest"].L == pad + 1 and by_id[f"{n}-short-T1"].L < n and by_id[f"{n}-short-T1"].L // (n // 4) == 1
    # backward: the tail cases have samples no frame reads, the quarter-hop ones have none
    by_id = {c.id: c for c in st.BACKWARD}
    for n in (512, 1024, 2048):
        c = by_id[f"{n}-tail"]
        assert c.L - st.first_untouched(c) == n // 4 - 1 and c.L % c.hop == c.hop - 1
        assert st.first_untouched(by_id[f"{n}-tail-quarter-hop"]) >= by_id[f"{n}-tail-quarter-hop"].L
        assert by_id[f"{n}-short-T1"].L < n and by_id[f"{n}-short-T1"].L // by_id[f"{n}-short-T1"].hop == 1


def test_backward_truth_against_finite_differences():
    """dy64 is the gradient of sum g mag; scale bounds it term by term and vanishes exactly where no frame reads"""
    c = st.Bwd("fd", 512, 256, 512, 5 * 256 + 255, 1)
    x, g = st.backward_inputs(c)
    dy, scale = st.backward64(c, x, g)
    assert bool((dy.abs() <= scale * (1 + 1e-12)).all())
    cut = st.first_untouched(c)
    assert cut < c.L and bool((scale[:, cut:] == 0).all()) and bool((scale[:, :cut] > 0).all())

    def loss(v):
        return float((st.mag64(st.frames64(v, 512, 512, 256)[0]) * g.double()).sum())
    for j in (0, 3, 127, 128, 700, cut - 1, cut):
        d = torch.zeros(1, c.L, dtype=torch.float64)
        d[0, j] = 1e-6
        fd = (loss(x.double() + d) - loss(x.double() - d)) / 2e-6
        # the loss is a sum of ~1e3: its float64 rounding over a step of 2e-6 leaves ~1e-7 on the difference quotient
        assert abs(fd - float(dy[0, j])) <= 1e-5 * float(scale[0, j]) + 2e-7, j
        assert (j >= cut) == (fd == 0.0 and float(dy[0, j]) == 0.0)
    e32 = ((st.backward32(c, x, g).double() - dy).abs()[:, :cut] / (st.EPS * scale[:, :cut])).max()
    assert float(e32) < 1e3                              # fp32 autograd is a few hundred eps at the very worst


def test_the_oracles_own_error_on_every_forward_case():
    """e_lin / e_mel of the fp32 oracle: finite everywhere, and of the size stft_truth's docstring claims"""
    worst_lin, worst_mel = (0.0, ""), (0.0, "")
    for c in st.FORWARD:
        x = st.signal(c)
        assert x.shape == (c.B, c.L) and x.dtype == torch.float32
        tr = st.truth(c, x)
        mel32, lin32 = st.oracle32(c, x)
        el, em = st.e_lin(lin32, tr["mag"], tr["norm"]), st.e_mel(mel32, tr["mag"], tr["norm"], tr["basis"])
        print(f"[stft oracle] {c.id}: e_lin {el:.2f} e_mel {em:.2f}")
        assert math.isfinite(el) and math.isfinite(em), c.id
        assert el < 200 and em < 200, c.id
        empty = ~(tr["basis"] != 0).any(dim=1)
        assert bool((mel32[:, empty] == torch.log(torch.tensor(1e-5))).all()), c.id
        worst_lin, worst_mel = max(worst_lin, (el, c.id)), max(worst_mel, (em, c.id))
    report(f"[stft oracle] worst e_lin {worst_lin[0]:.2f} ({worst_lin[1]}), worst e_mel {worst_mel[0]:.2f} ({worst_mel[1]})")
