"""CPU side of test_gpu_admm_degrees.py: the builders of admm_codes.py give what they are asked for, the tests' statement of the ADMM
decoder's dispatch (blocks of the stopping sums, eligibility of the LDS-resident kernel) matches hand-worked values, every decode case is
one where frames leave at many different iterations (so a device test of it cannot pass on frames that all behave alike), and the C oracle
reproduces the vectors captured from the reference's ADMM class on five of the new codes (oracle/make_goldens_admm.py --edge)."""
import numpy as np
import pytest

import admm_codes as AC
import admm_oracle as A


edge_cases, edge_arrays = AC.edge_cases, AC.edge_arrays


# ---- builders ---------------------------------------------------------------------------------------------------------------------------

def _no_duplicate_edge(code):
    key = code.edge_chk.astype(np.int64) * code.n + code.edge_var
    return len(np.unique(key)) == code.E and (np.diff(key) > 0).all()


@pytest.mark.parametrize("degrees,n", [(AC.CYCLE_0_8, 60), ([1] * 5, 8), ([1], 3), (AC.CYCLE_1_16, 120), ([17, 3, 3], 40), ([0, 0, 2, 0], 2)])
def test_rows_code_has_the_degrees_asked_for(degrees, n):
    code = AC.rows_code(degrees, n, 5)
    assert (code.m, code.n, code.E) == (len(degrees), n, sum(degrees))
    assert AC.check_degrees(code).tolist() == list(degrees) and _no_duplicate_edge(code)
    again, other = AC.rows_code(degrees, n, 5), AC.rows_code(degrees, n, 6)
    assert np.array_equal(again.edge_var, code.edge_var) and np.array_equal(again.edge_chk, code.edge_chk)
    if sum(degrees) > 5 and max(degrees) < n:
        assert not np.array_equal(other.edge_var, code.edge_var)


def test_cycling_degrees_hold_empty_rows_inside_and_last():
    assert AC.CYCLE_0_8[8] == 0 and AC.CYCLE_0_8[-1] == 0 and sorted(set(AC.CYCLE_0_8)) == list(range(9)) and len(AC.CYCLE_0_8) == 45
    assert sorted(set(AC.CYCLE_1_16)) == list(range(1, 17)) and len(AC.CYCLE_1_16) == 64
    code = AC.case_code("rows:cycle1_16")
    assert (code.E + code.n) % 128 != 0  # the repack case moves E + n rows in chunks of 128: the last chunk is a partial one


@pytest.mark.parametrize("L", sorted(AC.UNIFORM))
def test_uniform_codes_are_regular(L):
    n, l, r = AC.UNIFORM[L]
    code = AC.case_code("uniform:%d" % L)
    assert r == L and code.n == n and code.m == n * l // r and code.m < 128
    assert set(AC.check_degrees(code)) == {r} and set(AC.var_degrees(code)) == {l} and _no_duplicate_edge(code)
    assert AC.z_kernel_of(code) == "fixed<%d>" % L and AC.lds_plan(code) is None


@pytest.mark.parametrize("m,n", AC.LDS_SHAPES)
def test_dc6_code_degrees(m, n):
    code = AC.dc6_code(m, n, 11)
    dv = AC.var_degrees(code)
    assert (code.m, code.n, code.E) == (m, n, 6 * m) and set(AC.check_degrees(code)) == {6} and _no_duplicate_edge(code)
    assert dv.min() >= 1 and dv.max() <= 3
    assert (set(dv) == {3}) == ((m, n) in AC.LDS_ALL_DV3)
    if (m, n) not in AC.LDS_ALL_DV3 and (m, n) != (127, 300):
        assert set(dv) == {1, 2, 3}
    again = AC.dc6_code(m, n, 11)
    assert np.array_equal(again.edge_var, code.edge_var)


def test_dc6_code_bounds():
    for m, n in ((10, 19), (10, 61)):
        with pytest.raises(AssertionError):
            AC.dc6_code(m, n, 1)
    assert set(AC.var_degrees(AC.dc6_code(10, 60, 1))) == {1} and set(AC.var_degrees(AC.dc6_code(10, 20, 1))) == {3}


def test_planted_rows():
    code = AC.case_code("uniform:5")
    g = AC.planted_gamma(code, np.random.RandomState(3), 130, 3.0)
    P = AC.PLANTED
    assert g.shape == (130, code.n) and (g[P["zero"]] == 0).all() and (g[P["plus"]] == 1e6).all() and (g[P["minus"]] == -1e6).all()
    assert (g[P["alternating"]][0::2] == 1e6).all() and (g[P["alternating"]][1::2] == -1e6).all()
    assert (g[P["grid"]] / 0.75 == np.round(g[P["grid"]] / 0.75)).all() and len(np.unique(g[P["grid"]])) < code.n // 3
    assert np.isinf(g[P["inf"]]).all() and (g[P["inf"]] > 0).any() and (g[P["inf"]] < 0).any()
    rest = np.delete(g, sorted(P.values()), axis=0)
    assert np.isfinite(rest).all() and 0.8 < (rest > 0).mean() < 1.0  # the all-zero word: LLRs positive but for the noise
    assert np.array_equal(g, AC.planted_gamma(code, np.random.RandomState(3), 130, 3.0))
    one = AC.planted_gamma(code, np.random.RandomState(3), 1, 3.0)
    assert one.shape == (1, code.n) and np.isfinite(one).all() and (one != 0).all()  # a batch of one is a noise frame


# ---- the expected dispatch --------------------------------------------------------------------------------------------------------------

BY_HAND = {  # numpy's pairwise split worked by hand: halves rounded down to a multiple of 8 until a piece has at most 128 elements
    1: [1],
    128: [128],
    129: [64, 65],
    # 3600 = 1800 + 1800; 1800 = 896 + 904; 896 = 8 x 112; 904 = 448 + 456 = 4 x 112 + (224 + 232) = 4 x 112 + 2 x 112 + (112 + 120)
    3600: ([112] * 15 + [120]) * 2,
    # 4092 = 2040 + 2052; 2040 = 1016 + 1024; 1016 = 504 + 512 = (248 + 256) + 512 = (120 + 128) + 2 x 128 + 4 x 128; 1024 = 8 x 128
    # 2052 = 1024 + 1028; 1028 = 512 + 516; 516 = 256 + 260; 260 = 128 + 132; 132 = 64 + 68
    4092: [120] + [128] * 7 + [128] * 8 + [128] * 8 + [128] * 4 + [128] * 2 + [128, 64, 68],
}


@pytest.mark.parametrize("E", sorted(BY_HAND))
def test_leaves_of_against_a_split_by_hand(E):
    assert sum(BY_HAND[E]) == E
    assert AC.leaves_of(E) == len(BY_HAND[E]) and AC.blocks_of(E) == BY_HAND[E]


def test_blocks_reproduce_numpy_sum():
    # the split is numpy's: eight strided accumulators per block, block sums added back up the tree == ndarray.sum(), bit for bit
    rng = np.random.default_rng(5)
    for E in (7, 8, 9, 129, 136, 263, 1542, 3078, 3636, 4092):
        x = rng.standard_normal(E) ** 2 * 10.0 ** rng.uniform(-6, 2, E)
        sums, depth, o = [], [d for _, d in AC._split(E)], 0
        for n in AC.blocks_of(E):
            a = x[o:o + n]
            o += n
            if n < 8:
                s = -0.0
                for v in a:
                    s += v
            else:
                r = a[:8].copy()
                full = n - n % 8
                for i in range(8, full, 8):
                    r += a[i:i + 8]
                s = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
                for v in a[full:]:
                    s += v
            sums.append(s)
        while len(sums) > 1:  # the deepest adjacent pair of equal depth is a node's two children
            d = max(depth)
            i = depth.index(d)
            sums[i:i + 2], depth[i:i + 2] = [sums[i] + sums[i + 1]], [d - 1]
        assert 0.0 + sums[0] == x.sum()


LDS_TABLE = {(127, 300): None, (128, 256): (4, 1), (128, 512): (4, 1), (129, 400): (4, 1), (256, 512): (4, 1), (128, 513): None,
             (257, 514): (8, 1), (257, 1024): (8, 1), (512, 1024): (8, 1), (257, 1025): None, (513, 1026): (8, 2), (513, 1536): (8, 2),
             (513, 1537): None}


@pytest.mark.parametrize("m,n", AC.LDS_SHAPES)
def test_lds_plan_table(m, n):
    code = AC.case_code("dc6:%d,%d" % (m, n))
    assert AC.lds_plan(code) == LDS_TABLE[(m, n)]
    assert AC.z_kernel_of(code) == "fixed<6>"  # what the same code runs on under LDPC_ADMM_BACKEND=stream


def test_lds_plan_refuses_other_degrees():
    assert AC.lds_plan(AC.regular_code(1200, 3, 5, 1)) is None and AC.lds_plan(AC.regular_code(768, 4, 6, 1)) is None  # checks of 5; variables of 4
    code = AC.case_code("dc6:128,512")
    assert AC.lds_plan(AC.Code.from_edges(code.m, code.n + 1, code.edge_chk, code.edge_var)) is None  # a variable in no check


def test_lds_last_shape_is_set_by_the_lds_size_not_by_the_chains():
    """The rule `one lane per accumulator chain` (at most 32 blocks in eight waves) first fails at m = 642 (33 blocks); the largest m that
    keeps it is 680 (682: 33 blocks).  It never decides: at n = 1536 the frame's state is 240 m + 18256 bytes with 32 blocks, which passes
    160 KiB between m = 606 and 607, and n = 2 m, the smallest n, only moves that to 616 / 617.  So the pair at the edge of the LDS kernel is
    (606, 1536) / (607, 1536), and the pair at m* = 680 runs on the streaming kernels on both sides."""
    ms = AC.lds_mstar()
    assert ms == 680 and AC.leaves_of(6 * 600) == 32 and AC.leaves_of(6 * 682) == 33 and AC.leaves_of(6 * (ms + 1)) == 33
    assert min(m for m in range(513, 1025) if AC.leaves_of(6 * m) > 32) == 642
    assert AC.leaves_of(6 * 606) == 32 and 240 * 606 + 18256 <= AC.LDS_BYTES < 240 * 607 + 18256
    plans = {name: AC.lds_plan(AC.case_code(name)) for name in AC.lds_names()[len(AC.LDS_SHAPES):]}
    assert plans == {"dc6:606,1536": (8, 2), "dc6:607,1536": None, "dc6:680,1536": None, "dc6:681,1536": None}
    for m in range(513, 1025):  # whatever n: where the chains do not fit, the state does not either
        if AC.leaves_of(6 * m) > 32:
            assert 8 * (5 * 6 * m + 2 * m) > AC.LDS_BYTES


def test_z_kernel_of():
    want = {"rows:cycle0_8": "lds_arrays<8>", "rows:all1": "lds_arrays<8>", "rows:one_edge": "lds_arrays<8>", "rows:7_8": "lds_arrays<8>",
            "regular:99,3,9": "private<16>", "regular:96,4,16": "private<16>", "rows:cycle1_16": "private<16>", "rows:9_16": "private<16>",
            "rows:deg16": "private<16>"}
    for name, k in want.items():
        assert AC.z_kernel_of(AC.case_code(name)) == k, name
    assert set(AC.check_degrees(AC.case_code("rows:7_8"))) == {7, 8} and set(AC.check_degrees(AC.case_code("rows:9_16"))) == {9, 16}
    with pytest.raises(ValueError, match="check degree 17 above 16"):
        AC.z_kernel_of(AC.case_code("rows:deg17"))
    for E in AC.E_EDGES:
        code = AC.case_code("E:%d" % E)
        assert code.E == E and AC.check_degrees(code).max() <= 4 and 6 <= code.n <= 90
        assert AC.z_kernel_of(code) == "lds_arrays<8>" and AC.lds_plan(code) is None


@pytest.mark.parametrize("E", AC.E_EDGES)
def test_tail_rows_end_on_their_isolated_edge(E):
    """The last block of the stopping sums is the only ragged one at these E; its one-by-one tail (as far as edge_tail goes) lies on isolated
    edges, and row TAIL_ROW0 + j leaves at iteration 11 + j because of edge E - t + j alone: the same frame with +1e6 on that variable
    (the `plus` row) leaves at iteration 1.  A sum that loses or misplaces that element ends the frame ten iterations early."""
    code, t, blocks = AC.case_code("E:%d" % E), AC.edge_tail(E), AC.blocks_of(E)
    assert all(b % 8 == 0 for b in blocks[:-1]) and t == (1 if E == 1 else min(blocks[-1] % 8, E - 4)) and (t > 0) == (blocks[-1] % 8 > 0)
    assert code.E == E and code.n <= 90 and len(code.tail_vars) == t
    dc, dv = AC.check_degrees(code), AC.var_degrees(code)
    for j in range(t):
        k = E - t + j
        assert code.edge_var[k] == code.tail_vars[j] and dc[code.edge_chk[k]] == 1 and dv[code.edge_var[k]] == 1
    g = AC.case_gamma("E:%d" % E, 70)
    x, iters, conv = AC.oracle_of("E:%d" % E, 70, 60)
    assert iters[AC.PLANTED["plus"]] == 1 and conv[AC.PLANTED["plus"]]
    for j in range(t):
        f = AC.TAIL_ROW0 + j
        assert (np.delete(g[f], code.tail_vars[j]) == 1e6).all() and g[f, code.tail_vars[j]] == -AC.MU * (10.5 + j)
        assert iters[f] == 11 + j and conv[f] and (x[f] == 0).all()


# ---- exercise conditions ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,B,max_iter", AC.decode_cases(), ids=lambda v: str(v))
def test_case_is_worth_decoding(name, B, max_iter):
    """Frames leave at six or more different iteration counts and at least one through the stopping test, so a device that got the
    projection, a sum or the bookkeeping of leaving frames wrong would not agree with the oracle by having nothing to do.  The three codes
    without a check above degree 1 cannot do that at any SNR: every projection is 0, a variable is the scalar recursion
    x <- clip(-lambda / mu - gamma / mu), and it ends after about 1 + max(-gamma) / mu steps -- 1, 2 or 3 at these LLRs, or the cap on the
    -1e6 rows.  They are held to: more than one count, a converged frame and a capped one."""
    assert max_iter >= 60
    x, iters, conv = AC.oracle_of(name, B, max_iter)
    assert conv.any()
    if name in AC.DEGENERATE:
        assert AC.check_degrees(AC.case_code(name)).max() == 1
        assert len(np.unique(iters)) >= 2 and (iters == max_iter).any()
    else:
        assert len(np.unique(iters)) >= 6, np.unique(iters)
    planted = [f for f in AC.PLANTED.values() if f < B]
    assert len(planted) == 6 and np.isfinite(np.delete(x, planted, axis=0)[:, AC.var_degrees(AC.case_code(name)) > 0]).all()


# ---- what no decode can tell apart --------------------------------------------------------------------------------------------------------

def test_equal_projection_inputs_get_equal_outputs():
    """Why no planted row separates a stable sort from an unstable one in the projection: everything it computes after the sort (mass, r,
    facet, break points, beta) is a function of the sorted VALUES; the order of equal entries decides only which of them sits left of position
    r, and entries that tie across r come out equal (the projection onto a permutation-symmetric set keeps ties; here bit for bit).  So a
    compare-exchange that swaps equal values changes no output.  Held on tie-rich vectors for every length: equal inputs give equal outputs,
    and permuting the input permutes the output."""
    rng = np.random.default_rng(7)
    for L in range(2, 17):
        for t in range(1500):
            if t % 3 == 0:
                v = np.round(rng.uniform(-0.5, 1.5, L) * 4) / 4
            elif t % 3 == 1:
                v = rng.choice([0.0, 1.0, 0.5, 0.25, 0.75, 1.5, -0.5, 0.9, 0.6], L)
            else:
                v = rng.choice(rng.uniform(-0.3, 1.3, 3), L)
            p, perm = A.pp_project(v), rng.permutation(L)
            assert np.array_equal(A.pp_project(v[perm]), p[perm]), v
            assert all(len(np.unique(p[v == u])) == 1 for u in np.unique(v)), v


# ---- the oracle as a whole decoder against the reference on the new degrees ---------------------------------------------------------------

def test_edge_vectors_cover_the_five_codes():
    cases = edge_cases()
    assert [c["code"] for c in cases] == AC.GOLDEN_CODES
    kernels = [AC.z_kernel_of(AC.case_code(c["code"])) for c in cases]
    assert kernels == ["fixed<3>", "fixed<7>", "lds_arrays<8>", "private<16>", "fixed<6>"] and AC.lds_plan(AC.case_code(cases[4]["code"])) == (4, 1)


@pytest.mark.parametrize("case", edge_cases(), ids=lambda c: c["code"])
def test_builder_has_not_drifted_from_the_captured_code(case):
    a, code = edge_arrays(case), AC.case_code(case["code"])
    assert a["shape"].tolist() == [code.m, code.n]
    assert np.array_equal(a["chk"], code.edge_chk) and np.array_equal(a["var"], code.edge_var)


@pytest.mark.parametrize("case", edge_cases(), ids=lambda c: c["code"])
def test_admm_oracle_reproduces_reference_on_edge_codes(case):
    a = edge_arrays(case)
    x, iters, conv = A.admm_decode(AC.Graph(AC.case_code(case["code"])), a["gamma"], case["mu"], case["eps"], case["max_iter"])
    assert a["gamma"].shape[0] == case["frames"] == 30
    assert np.array_equal(iters, a["iters"])
    assert np.array_equal(A.pseudo_to_cw(x, case["allow_pseudo"]), a["xhat"])
    assert ((iters < case["max_iter"]) == (conv == 1)).all() and len(np.unique(iters)) >= 6
