"""Binary erasure channel and its message-passing decoder -- mirror of the reference's ``src/bec.py:11-18,70-125``.

Behind the ``bec`` selector ``SPA`` and ``MSA`` are the same ternary {-1,0,+1} erasure decoder (not ``bpa``), with
the stopping-set exit of src/bec.py:120; symbols are {0, 1, 2 = erased}.
"""
import numpy as np

from . import admm, hard, layered, qc, registry
from ._device import DecoderHandle, as_code


class Channel:
    name = "bec"

    def __init__(self, p):
        self.param = self.p = p

    def send(self, x):
        tt = (np.random.random(x.shape) < self.p).astype(int)  # src/bec.py:17-18
        return np.clip(x + tt * 10, 0, 2)


class SPA:
    id_keys = ["max_iter"]
    channel = "bec"

    def __init__(self, p, _code, **kwargs):
        self.param = p
        self.max_iter = kwargs["max_iter"]
        self.code = as_code(_code)
        self.precision = "f32"  # integer arithmetic; the field only selects staging widths
        self.handle = DecoderHandle(self.code, "BEC", "f32", kwargs.get("backend") or "auto", kwargs.get("device"))
        self.last_iters = None

    def decode(self, y):
        y = np.asarray(y)
        xhat, iters = self.handle.decode_host(None, y, self.max_iter)
        self.last_iters = iters
        return xhat[0].astype(np.int64)

    def decode_batch(self, y):
        if hasattr(y, "is_cuda"):
            out = self.handle.decode_device(None, y, self.max_iter)
        else:
            out = self.handle.decode_host(None, y, self.max_iter)
        self.last_iters = out[1]
        return out


class MSA(SPA):
    pass


registry.add_bec_refusals(globals())  # NMSA, LMSA, QMSA, OSD: NotImplementedError, the sentence is the registry's


class GALB:
    """Gallager-B decodes hard decisions; the erasure channel delivers none for an erased symbol."""
    id_keys = hard.GALB.id_keys

    def __init__(self, *a, **k):
        raise NotImplementedError("decoder GALB (hard-decision Gallager-B) does not exist over the bec: a hard-decision decoder has no erasures "
                                  "to work on; use SPA / MSA (peeling) or ML there")


class LQMSA:
    """Layered fixed-point min-sum quantises and scales magnitudes; the ternary erasure decoder has none."""
    id_keys = layered.LQMSA.id_keys

    def __init__(self, *a, **k):
        raise NotImplementedError("decoder LQMSA (layered fixed-point min-sum) does not exist over the bec: the erasure decoder has no "
                                  "magnitudes to quantise; use SPA / MSA there")


class SLQMSA:
    """The streaming layered fixed-point min-sum quantises and scales magnitudes as LQMSA does; the ternary erasure decoder has none."""
    id_keys = layered.SLQMSA.id_keys

    def __init__(self, *a, **k):
        raise NotImplementedError("decoder SLQMSA (streaming layered fixed-point min-sum) does not exist over the bec: the erasure decoder "
                                  "has no magnitudes to quantise; use SPA / MSA there")


class QCMSA:
    """The quasi-cyclic layered fixed-point min-sum quantises and scales magnitudes as LQMSA does; the ternary erasure decoder has none."""
    id_keys = qc.QCMSA.id_keys

    def __init__(self, *a, **k):
        raise NotImplementedError("decoder QCMSA (quasi-cyclic layered fixed-point min-sum) does not exist over the bec: the erasure decoder "
                                  "has no magnitudes to quantise; use SPA / MSA there")


class ADMM:  # src/bec.py:38-45,58-62: LLR wrapper with +-1e8 for the known symbols, 0 for an erasure
    id_keys = admm.ADMM.id_keys
    channel = "bec"

    def __init__(self, p, _code, **kwargs):
        self.param, self.dec, safe_inf = p, admm.ADMM(_code, **kwargs), 1e8
        self.llr = np.array([safe_inf, -safe_inf, 0])  # 0 WP1, 1 WP1, 0 OR 1 WP0.5
        self.stats = self.dec.stats

    def decode(self, y):
        return self.dec.decode(y, self.llr[np.asarray(y)])

    def decode_batch(self, y):
        return self.dec.decode_batch(self.llr[np.asarray(y)])


class ML:  # src/bec.py: class ML
    """A code with a code book (the built-in toy codes): the code-book search ``ml.BecML``.  Every other code: peeling + GF(2)
    elimination of the residual system on the GPU (``bec_ml.BecEliminationML``).  Both pick uniformly among the maximisers."""
    id_keys = []

    def __new__(cls, p, _code, **kwargs):
        if getattr(_code, "gen_mtx", None) is not None:
            return BecML(p, _code, **kwargs)
        return BecEliminationML(p, _code, **kwargs)


from .bec_ml import BecEliminationML  # noqa: E402
from .ml import BecML  # noqa: E402
