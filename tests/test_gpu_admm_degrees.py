"""The ADMM decoder's kernels (csrc/ldpc_admm.hip) at every check degree and at the shape edges of its dispatch, against the C oracle
(oracle/admm_oracle.c): estimates, iteration counts and convergence flags of EVERY frame, bit for bit.

The shipped code files have check degrees {6}, {4}, {4, 6} and {2, 3}; the codes of admm_codes.py reach what those do not:
k_admm_z_fixed<2..8> (A), k_admm_z<8, LDS arrays> at degrees 0, 1, 5, 7, 8 (B), k_admm_z<16, private arrays> (C), the refusal above 16 (D),
the leaf / stack program of the stopping sums where its structure changes (E), the three instantiations of k_admm_lds with variables of one,
two and three checks on both sides of every eligibility rule (F), the repack with E + n no multiple of its chunk (G), the batch limit (H).
Each case asserts the kernel it claims to reach (admm_codes.z_kernel_of / lds_plan against AdmmHandle.last_backend()).  Every batch holds
the planted rows of admm_codes.planted_gamma; test_admm_codes_cpu.py holds that frames of each case leave at many different iterations."""
import numpy as np
import pytest

import admm_codes as AC
import admm_oracle as A

pytestmark = pytest.mark.gpu


def _decode(code, gamma, max_iter=AC.MAX_ITER):
    """A fresh handle -> (x, iters, converged) as numpy, last_backend(), last_repacks()."""
    import torch
    from ldpc_decoders_amd._device import AdmmHandle

    h = AdmmHandle(code)
    x, it, cv = h.decode_device(torch.from_numpy(gamma).cuda(), AC.MU, AC.EPS, max_iter)
    return (x.cpu().numpy(), it.cpu().numpy(), cv.cpu().numpy()), h.last_backend(), h.last_repacks()


def _same(got, want, frames=None):
    s = slice(None, frames)
    assert np.array_equal(got[1][s], want[1][s]), "iteration counts, first at frame %d" % np.flatnonzero(got[1][s] != want[1][s])[0]
    assert np.array_equal(got[2][s], want[2][s])
    assert np.array_equal(got[0][s], want[0][s], equal_nan=True)


def _streaming_case(name, kernel, B=AC.B, max_iter=AC.MAX_ITER):
    code = AC.case_code(name)
    assert AC.z_kernel_of(code) == kernel and AC.lds_plan(code) is None
    got, backend, _ = _decode(code, AC.case_gamma(name, B), max_iter)
    assert backend == "stream"
    _same(got, AC.oracle_of(name, B, max_iter))


# ---- A: one check degree, 2..8 ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("L", sorted(AC.UNIFORM))
def test_uniform_check_degree(L):
    _streaming_case("uniform:%d" % L, "fixed<%d>" % L)


@pytest.mark.parametrize("L", [3, 7])
@pytest.mark.parametrize("B,max_iter", [(1, 100), (64, 100), (65, 100), (130, 1), (130, 0)])
def test_odd_degree_batch_and_cap_edges(L, B, max_iter):
    # one frame, a full tile, a tile and one frame; every frame out through the cap after one iteration; no cap at all
    _streaming_case("uniform:%d" % L, "fixed<%d>" % L, B, max_iter)


# ---- B: unequal degrees up to 8 ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["rows:cycle0_8", "rows:all1", "rows:one_edge", "rows:7_8"])
def test_unequal_degrees_up_to_8(name):
    _streaming_case(name, "lds_arrays<8>")


# ---- C: degrees 9..16 -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["regular:99,3,9", "regular:96,4,16", "rows:cycle1_16", "rows:9_16"])
def test_degrees_9_to_16(name):
    _streaming_case(name, "private<16>")


# ---- D: degree 17 -----------------------------------------------------------------------------------------------------------------------

def test_check_degree_17_is_refused_and_16_accepted():
    from ldpc_decoders_amd import admm
    from ldpc_decoders_amd._device import AdmmHandle
    from ldpc_decoders_amd._lib import LdpcHipError

    code = AC.case_code("rows:deg17")
    assert AC.check_degrees(code).tolist() == [17, 3, 3]
    for make in (lambda: AdmmHandle(code), lambda: admm.ADMM(code, mu=AC.MU, eps=AC.EPS, max_iter=10, allow_pseudo=0)):
        with pytest.raises(LdpcHipError, match=r"error -4: .*check degree 17 above 16"):
            make()
    assert AC.check_degrees(AC.case_code("rows:deg16")).tolist() == [16, 3, 3]
    _streaming_case("rows:deg16", "private<16>")


# ---- E: the summation program of the stopping test ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("E", AC.E_EDGES)
def test_stopping_sums_at_the_edges_of_the_leaf_program(E):
    """E around 8 (a block below eight elements is added one by one from -0.0), 16 (the first full round of the eight accumulators), 128 /
    129 (one block / the first split, 64 + 65), 136, 257 and 263 (blocks with a tail of 1..7 elements behind the strided part).
    What this sees: rows TAIL_ROW0.. of each batch (admm_codes.tail_rows) leave at iteration 11 + j because of ONE element of the sums,
    the j-th of the elements that the last block adds one by one behind its accumulators (an isolated edge: every other squared distance is
    exactly 0 by then), so a block that loses, repeats or misplaces one of those elements ends that frame ten iterations early; E = 8, 16,
    128 and 136 have no such elements.  The noise frames see a block or a stack program that is grossly wrong.  What it does not see: a
    pure reordering of the additions, which moves a sum by an ulp and shows only in a frame within that ulp of the threshold (the order
    is held on the CPU: test_oracle_admm.test_numpy_sum_order, test_admm_codes_cpu.test_blocks_reproduce_numpy_sum)."""
    name = "E:%d" % E
    assert AC.case_code(name).E == E and AC.leaves_of(E) == (1 if E <= 128 else 2 if E <= 256 else 3)
    _streaming_case(name, "lds_arrays<8>", 70, 60)


# ---- F: the LDS-resident kernel ------------------------------------------------------------------------------------------------------------

def _lds_case(name, monkeypatch, B=AC.B, max_iter=AC.MAX_ITER, with_oracle=None):
    code = AC.case_code(name)
    plan = AC.lds_plan(code)
    gamma = AC.case_gamma(name, B)
    monkeypatch.delenv("LDPC_ADMM_BACKEND", raising=False)
    got, backend, _ = _decode(code, gamma, max_iter)
    assert backend == ("lds" if plan else "stream")
    if plan:
        monkeypatch.setenv("LDPC_ADMM_BACKEND", "stream")
        stream, backend, _ = _decode(code, gamma, max_iter)
        assert backend == "stream" and AC.z_kernel_of(code) == "fixed<6>"
        _same(got, stream)
    if with_oracle is None:
        _same(got, AC.oracle_of(name, B, max_iter))
    else:
        _same(got, A.admm_decode(AC.Graph(code), gamma[:with_oracle], AC.MU, AC.EPS, max_iter), with_oracle)
    return plan


@pytest.mark.parametrize("name", AC.lds_names())
def test_lds_kernel_shapes(name, monkeypatch):
    """k_admm_lds<6,3,2,4,1> (m <= 256), <6,3,2,8,1> (m <= 512), <6,3,3,8,2> (m <= 1024) and the codes one step outside each rule: LDS ==
    streaming kernels == oracle on all frames.  (A check of six edges has no isolated edge: the single elements of this kernel's own block
    sums are not held one by one as in section E, only through frames that happen to sit near the threshold.)  The last four names: the (606, 1536) / (607, 1536) pair on either side of the 160 KiB rule,
    and the pair at the largest m with 32 blocks, which that rule has sent to the streaming kernels already
    (test_admm_codes_cpu.test_lds_last_shape_is_set_by_the_lds_size_not_by_the_chains)."""
    _lds_case(name, monkeypatch)


@pytest.mark.parametrize("B,max_iter,with_oracle", [(1, 100, None), (700, 100, 64), (130, 1, None), (130, -1, None)])
def test_lds_kernel_8_waves_one_pass_batches_and_caps(B, max_iter, with_oracle, monkeypatch):
    # one frame (one workgroup); more frames than workgroups in flight; out through the cap after one iteration; no cap
    assert _lds_case("dc6:257,1024", monkeypatch, B, max_iter, with_oracle) == (8, 1)


# ---- G: repack ---------------------------------------------------------------------------------------------------------------------------

def test_repack_with_degrees_1_to_16_is_bit_transparent(monkeypatch):
    name, B = "rows:cycle1_16", AC.REPACK_B
    code = AC.case_code(name)
    assert (code.E + code.n) % 128 != 0 and AC.z_kernel_of(code) == "private<16>"
    gamma = AC.case_gamma(name, B)
    monkeypatch.setenv("LDPC_ADMM_BACKEND", "stream")
    monkeypatch.setenv("LDPC_STREAM_REPACK", "0")
    monkeypatch.delenv("LDPC_STREAM_REPACK_FILL", raising=False)
    off, _, repacks_off = _decode(code, gamma)
    monkeypatch.setenv("LDPC_STREAM_REPACK", "1")
    monkeypatch.setenv("LDPC_STREAM_REPACK_FILL", "0.95")
    on, _, repacks_on = _decode(code, gamma)
    assert repacks_off == 0 and repacks_on >= 1
    _same(on, off)
    _same(off, AC.oracle_of(name, B, AC.MAX_ITER))


# ---- H: batch limit ------------------------------------------------------------------------------------------------------------------------

def test_batch_above_the_tile_grid_is_refused():
    import torch
    from ldpc_decoders_amd._device import AdmmHandle
    from ldpc_decoders_amd._lib import LdpcHipError

    code = AC.case_code("rows:one_edge")
    gamma = torch.zeros((65535 * 64 + 1, code.n), dtype=torch.float64, device="cuda")
    with pytest.raises(LdpcHipError, match=r"error -1: .*at most"):
        AdmmHandle(code).decode_device(gamma, AC.MU, AC.EPS, 10)


# ---- the new degrees against vectors captured from the reference's ADMM class ---------------------------------------------------------------

@pytest.mark.parametrize("case", AC.edge_cases(), ids=lambda c: c["code"])
def test_admm_bit_exact_vs_reference_on_edge_codes(case):
    from ldpc_decoders_amd import admm

    a = AC.edge_arrays(case)
    dec = admm.ADMM(AC.case_code(case["code"]), mu=case["mu"], eps=case["eps"], max_iter=case["max_iter"], allow_pseudo=case["allow_pseudo"])
    est, iters = dec.decode_batch(a["gamma"])
    assert np.array_equal(iters, a["iters"])
    assert np.array_equal(np.asarray(est), a["xhat"])
    assert dec.stats()["iter"] == np.bincount(a["iters"], minlength=2000).tolist()
    assert dec.handle.last_backend() == ("lds" if AC.lds_plan(dec.code) else "stream")
