"""The state machine of the streaming sweep loop (csrc/ldpc_tiles.hpp, SweepPolls): the poll ring, the drain, the exit when every frame
has left, the repack decided on a poll that has a newer one pending behind it, and the repack policy's clamp -- on the four drivers of the
loop: fp32 min-sum on the streaming backend and fp32 layered min-sum (run<T, ALG>), the fp16 storage mode (run16<ALG>) and SLQMSA at its
default fixed point (run_chunk<T>).  Code 1200_3_6_rand_ldpc_1.  Every case compares a decode with the same decode under
LDPC_STREAM_REPACK=0 -- decisions, iteration counts, sweeps -- and, where an exact oracle exists, with the oracle: the C oracle for min-sum,
lmsa_oracle.py for layered min-sum, lqmsa_oracle.py for SLQMSA (the fp16 mode has none: test_gpu_repack.py compares it the same way).

The batches draw their frames from a small pool (64 frames at 7 dB, which the oracles decode within 3 sweeps, and 6 frames of pure noise
of unit variance -- small LLRs that survive SLQMSA's quantiser step of 1/4 -- which the oracles run to sweep 200), so the oracles decode 70
frames once and every frame of a batch is still compared.  The noise frames are scattered so that each of the 13 tiles keeps one.

`last_sweeps` of a decode that ends because every frame has left is the sweep count of the POLL that saw the batch empty -- not the
oracle's last sweep (the oracle looks after every sweep, the loop every poll_every-th) and not the loop's own count when it reads that
poll (it has enqueued up to a further block of sweeps by then): the first multiple of poll_every at or beyond the last frame's iteration
count, poll_every by the rules of ldpc_tiles.hpp / run16 (13 tiles: 11 for fp32, 15 for SLQMSA, 4 for fp16 storage)."""
import numpy as np
import pytest

import bp_oracle as O
import c_oracle as C
import lmsa_oracle as L
import lqmsa_oracle as LQ

pytestmark = pytest.mark.gpu
NAME = "1200_3_6_rand_ldpc_1"
DRIVERS = ["msa_f32", "lmsa_f32", "msa_f16", "slq"]
B_BIG = 64 * 12 + 3
N_EASY, N_HARD = 64, 6
_CACHE = {}


def _code():
    from ldpc_decoders_amd import codes

    if "code" not in _CACHE:
        c = codes.get_code(NAME)
        _CACHE["code"] = (O.Edges(c.m, c.n, c.edge_chk, c.edge_var), c)
    return _CACHE["code"]


def _pool():
    """fp32 priors [N_EASY + N_HARD, n]: the frames at 7 dB first, then the noise frames"""
    if "pool" not in _CACHE:
        g = _code()[0]
        rng = np.random.RandomState(47)
        easy = O.biawgn_priors(-1 + rng.normal(0, np.sqrt(O.biawgn_noise_var(7.0)), (N_EASY, g.n)), 7.0)
        _CACHE["pool"] = np.ascontiguousarray(np.concatenate([easy, rng.standard_normal((N_HARD, g.n))]).astype(np.float32))
    return _CACHE["pool"]


def _mixed():
    """row of the pool per frame of the case-1 batch: about one frame in ten is a noise frame, every tile keeps at least one"""
    rng = np.random.RandomState(5)
    idx = rng.randint(0, N_EASY, B_BIG)
    hard = rng.permutation(B_BIG)[:B_BIG // 10]
    hard = np.union1d(hard, np.arange(13) * 64 + rng.randint(0, 3, 13))  # (the last tile holds three frames)
    idx[hard] = N_EASY + rng.randint(0, N_HARD, hard.size)
    return idx


def _all_easy(B):
    return np.random.RandomState(6).randint(0, N_EASY, B)


def _oracle(driver, cap):
    """(xhat, iters) of the pool, or None for the fp16 storage mode"""
    key = ("oracle", driver, cap)
    if key not in _CACHE:
        g, pri = _code()[0], _pool()
        if driver == "msa_f32":
            got = C.bp_decode(g, "MSA", None, pri, cap, dtype=np.float32)
        elif driver == "lmsa_f32":
            got = L.lmsa_decode(g, None, pri, cap, 1.0, 0.0, dtype=np.float32)
        elif driver == "slq":
            got = LQ.lqmsa_decode(g, None, pri, cap)
        else:
            got = None
        _CACHE[key] = None if got is None else (got[0], got[1])
    return _CACHE[key]


def _handle(driver):
    from ldpc_decoders_amd._device import DecoderHandle, SlqHandle

    c = _code()[1]
    if driver == "slq":
        return SlqHandle(c)
    alg, prec = driver.split("_")
    return DecoderHandle(c, alg.upper(), prec, "stream")


def _decode(h, idx, cap):
    """-> (xhat, iters, last sweeps, repacks)"""
    import torch

    pri = torch.from_numpy(_pool()[idx]).cuda()
    x, it = h.decode_device(pri, None, cap)[:2]
    x, it = x.cpu().numpy(), it.cpu().numpy()
    if hasattr(h, "last_repacks"):
        assert h.last_stats()[0] == "stream"
        return x, it, h.last_stats()[1], h.last_repacks()
    sweeps, repacks, chunks = h.last_stats()
    assert chunks == 1
    return x, it, sweeps, repacks


def _env(monkeypatch, **env):
    for k in ("LDPC_STREAM_REPACK", "LDPC_STREAM_REPACK_FILL"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv("LDPC_STREAM_" + k, v)


def _off(monkeypatch, driver, which, idx, cap):
    """the decode with the repack switched off, once per (driver, batch)"""
    key = ("off", driver, which, cap)
    if key not in _CACHE:
        _env(monkeypatch, REPACK="0")
        _CACHE[key] = _decode(_handle(driver), idx, cap)
        assert _CACHE[key][3] == 0
    return _CACHE[key]


def _same(got, want, where):
    assert np.array_equal(got[1], want[1]), (where, np.flatnonzero(got[1] != want[1])[:8])
    assert np.array_equal(got[0], want[0]), (where, np.flatnonzero((got[0] != want[0]).any(axis=1))[:8])


def _poll_every(driver, tiles):
    """the poll cadence of the driver's loop for a bounded run of `tiles` tiles of this code"""
    g = _code()[0]
    E, n = len(g.var), g.n
    if driver == "msa_f16":
        return 1 if tiles * 64.0 * (8.0 * E + 4.0 * n) / 5.0e6 > 1500.0 else 4
    bytes_per_frame = 6.0 * E + 2.0 * n if driver == "slq" else 4 * (4.0 * E + n)
    return min(max(int(300.0 / (15.0 + tiles * 64.0 * bytes_per_frame / 5.0e6)), 1), 16)


def _check_recipe(driver, cap, it_easy, it_hard):
    """the pool does what the cases are built on: the 7 dB frames have left before the first poll, the noise frames run to the cap"""
    assert it_easy.max() < _poll_every(driver, 13) and it_easy.max() <= 3, (driver, it_easy.max())
    if it_hard is not None:
        assert (it_hard == cap).all(), (driver, it_hard)


# ---------------------------------------------------------------------------------------------- 1. ring wrap, repack behind a pending poll
@pytest.mark.parametrize("driver", DRIVERS)
def test_ring_wrap_and_a_repack_while_a_poll_is_pending(driver, monkeypatch):
    """200 sweeps of 13 tiles: 13 (SLQMSA), 18 (fp32) or 49 (fp16 storage) polls through a ring of four slots; the noise frames are fewer than 0.95 of their
    tiles at the first poll, which the ring loops read when the second is enqueued behind it -- the repack leaves that one stale."""
    idx, cap = _mixed(), 200
    hard = idx >= N_EASY
    assert all(hard[t * 64:(t + 1) * 64].any() for t in range(13)) and 0.85 < 1 - hard.mean() < 0.92
    want = _oracle(driver, cap)
    off = _off(monkeypatch, driver, "mixed", idx, cap)
    _env(monkeypatch, REPACK_FILL="0.95")
    got = _decode(_handle(driver), idx, cap)
    print("%s: sweeps %d, repacks %d (off: %d)" % (driver, got[2], got[3], off[3]))
    assert got[2] == off[2] == cap and got[3] >= 1 and off[3] == 0
    _same(got, off, (driver, "eager against off"))
    if want is None:
        _check_recipe(driver, cap, got[1][~hard], got[1][hard])
    else:
        _check_recipe(driver, cap, want[1][:N_EASY], want[1][N_EASY:])
        _same(got, (want[0][idx], want[1][idx]), (driver, "oracle"))


# ---------------------------------------------------------------------------------------------- 2. everything leaves between polls
@pytest.mark.parametrize("driver", DRIVERS)
def test_every_frame_leaves_between_two_polls(driver, monkeypatch):
    """Every frame has left after three sweeps; the loop learns it from the first poll, which the ring loops read a block of sweeps later."""
    idx, cap = _all_easy(B_BIG), 50
    want = _oracle(driver, cap)
    off = _off(monkeypatch, driver, "easy", idx, cap)
    _env(monkeypatch, REPACK_FILL="0.95")
    got = _decode(_handle(driver), idx, cap)
    _same(got, off, (driver, "eager against off"))
    last = (want[1][idx] if want is not None else got[1]).max()
    _check_recipe(driver, cap, want[1][:N_EASY] if want is not None else got[1], None)
    every = _poll_every(driver, 13)
    print("%s: last frame left after %d sweeps, poll every %d, sweeps reported %d" % (driver, last, every, got[2]))
    assert got[2] == off[2] == every * -(-last // every) and got[3] == 0
    if want is not None:
        _same(got, (want[0][idx], want[1][idx]), (driver, "oracle"))


# ---------------------------------------------------------------------------------------------- 3. one tile, the unbounded run
@pytest.mark.parametrize("B", [37, 64 * 3 + 1])
@pytest.mark.parametrize("driver", DRIVERS)
def test_the_unbounded_run_ends_on_its_own(driver, B, monkeypatch):
    """max_iter = 0 polls at every sweep and reads each poll at once (fp16 storage: at its own cadence); one tile reads at once anyway."""
    idx = _all_easy(B)
    _env(monkeypatch)
    h = _handle(driver)
    bounded = _decode(h, idx, 50)
    free = _decode(h, idx, 0)
    _same(free, bounded, (driver, B))
    if driver != "msa_f16":  # a poll at every sweep: the sweep count is that of the last frame to leave
        assert free[2] == free[1].max()
    want = _oracle(driver, 50)
    if want is not None:
        _same(free, (want[0][idx], want[1][idx]), (driver, B, "oracle"))


# ---------------------------------------------------------------------------------------------- 4. a hostile fill
@pytest.mark.parametrize("fill", ["-1", "nan"])
@pytest.mark.parametrize("driver", DRIVERS)
def test_a_negative_or_nan_fill_never_repacks(driver, fill, monkeypatch):
    idx, cap = _mixed(), 200
    off = _off(monkeypatch, driver, "mixed", idx, cap)
    _env(monkeypatch, REPACK_FILL=fill)
    got = _decode(_handle(driver), idx, cap)
    assert got[3] == 0 and got[2] == off[2] == cap
    _same(got, off, (driver, fill))


# ---------------------------------------------------------------------------------------------- 5. both output forms on the repacked path
def test_bytes_and_words_in_one_repacked_slqmsa_call(monkeypatch):
    """ldpc_slq_decode writes whichever of xhat / bits it is handed, at the repack and at the end: both in one call equal the two alone."""
    import torch

    from ldpc_decoders_amd import _lib

    idx, cap = _mixed(), 200
    _env(monkeypatch, REPACK_FILL="0.95")
    h = _handle("slq")
    pri = torch.from_numpy(_pool()[idx]).cuda()
    x2, it2, w2 = h.decode_device(pri, None, cap, bits=True)
    assert h.last_stats()[1] >= 1
    x1, it1 = h.decode_device(pri, None, cap)
    assert h.last_stats()[1] >= 1
    w1, it3 = torch.full_like(w2, -1), torch.empty_like(it2)
    # words alone: the C entry point without a byte output
    _lib.check(h._fn("decode")(h.h, _lib.DTYPE["f32"], pri.data_ptr(), None, len(idx), cap, 0, None, w1.data_ptr(), it3.data_ptr(), None,
                               torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert h.last_stats()[1] >= 1
    assert torch.equal(x2, x1) and torch.equal(w2, w1) and torch.equal(it2, it1) and torch.equal(it2, it3)
    assert np.array_equal(w2.cpu().numpy().view(np.uint32), LQ.pack_words(x2.cpu().numpy()))
