"""Hard-decision decoding: bit-sliced Gallager-B (no upstream counterpart -- every decoder of the reference works on soft values,
src/bpa.py, or on erasures, src/bec.py).  One bit per message, the received word ``y`` in {0,1}^n in, a word and an iteration count out;
the contract is the ``ldpc_hard_*`` block of include/ldpc_hip.h."""
import numpy as np

from ._device import HardHandle, as_code

LDS_BYTES = 160 * 1024


def hard_lds_bytes(m, n, E):
    """LDS bytes one slab of 32 frames takes in the LDS-resident kernel (csrc/ldpc_hard.hpp hard_lds_bytes): y, x, v2c, the check
    parities and 4 words of slab state.  The kernel exists for a code iff this is at most ``LDS_BYTES``."""
    return 4 * (2 * n + E + m + 4)


def flip_threshold(d, t):
    """b_d of the contract: the number of disagreeing extrinsic messages that flips a message of a variable of degree ``d``."""
    d = np.asarray(d)
    if t == 0:
        return np.maximum(d - 1, 0) // 2 + 1
    return np.minimum(t, np.maximum(d - 1, 1))


def check_params(max_iter, gal_threshold):
    """What ``ldpc_hard_decode`` / ``ldpc_hard_set_threshold`` accept, checked before a decoder exists -> (max_iter, t) as ints."""
    if max_iter is None or float(max_iter) != int(max_iter) or int(max_iter) < 1:
        raise ValueError("GALB needs max_iter >= 1: a hard-decision decoder may oscillate for ever and has no exit of its own (got %r)" % (max_iter,))
    t = 0 if gal_threshold is None else gal_threshold
    if float(t) != int(t) or not 0 <= int(t) <= 255:
        raise ValueError("gal_threshold is an integer in 0..255 (0: the majority of the extrinsic messages; got %r)" % (gal_threshold,))
    return int(max_iter), int(t)


class GALB:
    """Gallager-B on the received bits.  ``gal_threshold`` t = 0: a message flips when the majority of the other checks disagree with the
    received bit (Gallager A for degree 3); t >= 1: when at least min(t, d - 1) of them do.  ``decode`` / ``decode_batch`` take the
    received word(s) as numpy or CUDA uint8 in {0, 1}; ``last_iters`` holds the sweeps of the last call."""
    id_keys = ["max_iter", "gal_threshold"]

    def __init__(self, parity_mtx, max_iter=10, gal_threshold=0, backend="auto", **_):
        self.max_iter, self.gal_threshold = check_params(max_iter, gal_threshold)
        self.code = as_code(parity_mtx)
        self.precision = "f32"  # integer arithmetic; the field only selects the width of the BI-AWGN channel output
        self.handle = HardHandle(self.code, backend or "auto", _.get("device"), self.gal_threshold)
        self.last_iters = None

    @property
    def parity_mtx(self):
        return self.code.parity_mtx

    def _host(self, y):
        import torch

        y = np.ascontiguousarray(np.atleast_2d(y))
        if y.ndim != 2 or y.shape[1] != self.code.n:
            raise ValueError("frames must have n=%d entries" % self.code.n)
        if y.dtype.kind not in "biu" or ((y != 0) & (y != 1)).any():
            raise ValueError("GALB decodes hard decisions: integers in {0, 1}")
        yd = torch.from_numpy(y.astype(np.uint8)).to("cuda:%d" % self.handle.device)
        xhat, iters = self.handle.decode_device(yd, self.max_iter)
        return xhat.cpu().numpy(), iters.cpu().numpy()

    def decode(self, y):
        xhat, self.last_iters = self._host(np.asarray(y))
        return xhat[0].astype(np.int64)

    def decode_batch(self, y):
        """[B, n] frames -> (x_hat uint8 [B, n], iters int32 [B]).  numpy in -> numpy out; CUDA uint8 in -> CUDA tensors out."""
        if hasattr(y, "is_cuda"):
            out = self.handle.decode_device(y, self.max_iter)
        else:
            out = self._host(y)
        self.last_iters = out[1]
        return out
