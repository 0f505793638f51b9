"""BI-AWGN channel and its LLR decoders -- mirror of the reference's ``src/biawgn.py:10-42``."""
import numpy as np

from . import admm, hard, registry

noise_var = lambda snr_in_db: 10 ** (-snr_in_db / 10)  # noqa: E731  (src/biawgn.py:10)


class Channel:
    name = "biawgn"

    def __init__(self, snr_in_db):
        self.param = snr_in_db
        self.std_dev = np.sqrt(noise_var(snr_in_db))

    def send(self, x):  # {0,1} -> {-1,+1} + N(0, sigma); consumes numpy's global stream like upstream (src/biawgn.py:17-18)
        return (2 * x - 1) + np.random.normal(0, self.std_dev, x.shape)


class LLR:
    channel = "biawgn"

    def __init__(self, snr_in_db, dec):
        self.param, self.noise_var, self.dec = snr_in_db, noise_var(snr_in_db), dec

    def priors(self, y):
        return -2 * y / self.noise_var  # src/biawgn.py:28 ; positive == bit 0

    def decode(self, y):
        return self.dec.decode(y, self.priors(np.asarray(y)))

    def decode_batch(self, y):
        return self.dec.decode_batch(None if hasattr(y, "is_cuda") else y, self.priors(y))


class ADMM(LLR):  # src/biawgn.py:52-56
    id_keys = admm.ADMM.id_keys

    def __init__(self, snr_in_db, _code, **kwargs):
        super().__init__(snr_in_db, admm.ADMM(_code, **kwargs))
        self.stats = self.dec.stats

    def decode_batch(self, y):
        return self.dec.decode_batch(self.priors(np.asarray(y)))


class GALB(LLR):  # no upstream counterpart: Gallager-B on the observation sliced where the LLR is negative (bit 1 <=> prior < 0 <=> y > 0)
    id_keys = hard.GALB.id_keys

    def __init__(self, snr_in_db, _code, **kwargs):
        super().__init__(snr_in_db, hard.GALB(_code, **kwargs))

    def _slice(self, y):
        if hasattr(y, "is_cuda"):
            import torch

            return (self.priors(y) < 0).to(torch.uint8).contiguous()
        return (self.priors(np.asarray(y)) < 0).astype(np.uint8)

    def decode(self, y):
        return self.dec.decode(self._slice(y))

    def decode_batch(self, y):
        return self.dec.decode_batch(self._slice(y))


registry.add_llr_wrappers(globals(), LLR)  # SPA, MSA and this build's own (NMSA, QMSA, LMSA, OSD): LLR around the bpa class of that name

from .ml import BiawgnML as ML  # noqa: E402  (src/biawgn.py: class ML)
