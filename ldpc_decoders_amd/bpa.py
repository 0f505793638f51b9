"""Flooding belief propagation in the LLR domain on the GPU -- mirror of the reference's ``src/bpa.py``.

Same classes and call shapes: ``SPA(parity_mtx, max_iter=..)`` / ``MSA(parity_mtx, max_iter=..)`` (extra keyword
arguments are ignored, the reference splats all CLI flags into the constructor, src/main.py:26), ``id_keys``, and
``decode(y, priors) -> x_hat`` (src/bpa.py:17-63).  Added: ``decode_batch`` (many frames per call, numpy or CUDA
tensors).  The arithmetic is in libldpc_hip.so; this file only moves buffers.

Extra constructor keywords (all optional):
  precision  'f64' (default here: bit-exact min-sum against the reference) or 'f32' (throughput mode)
  backend    'auto' | 'stream' | 'fused'
  device     GPU ordinal (default: torch's current device, else 0)
"""
import numpy as np

from ._device import DecoderHandle, OsdHandle, as_code, check_correction, check_fixed_point, check_layers


class BPA:
    id_keys = ["max_iter"]
    alg = None

    def __init__(self, parity_mtx, **kwargs):
        self.max_iter = kwargs["max_iter"]  # KeyError if absent, as upstream (src/bpa.py:10)
        self.code = as_code(parity_mtx)
        self.precision = kwargs.get("precision") or "f64"
        self.handle = DecoderHandle(self.code, self.alg, self.precision, kwargs.get("backend") or "auto", kwargs.get("device"))
        self.last_iters = None

    @property
    def parity_mtx(self):
        return self.code.parity_mtx

    def _iter0_word(self, y):
        """Hard word for the iteration-0 syndrome check (src/bpa.py:20,29), or None when it cannot pass.

        Upstream tests ``(H @ y) % 2 == 0`` on the RAW received vector: meaningful for the BSC (y in {0,1}); for a
        real-valued BI-AWGN observation it passes only if every check sum is an even integer, which requires an
        integer-valued y -- handled here on the host only in that (measure-zero) case."""
        y = np.asarray(y)
        if y.dtype.kind == "f" and y.size and y.flat[0] != np.floor(y.flat[0]):
            return None, None  # a real-valued observation (every BI-AWGN frame): decided on the first entry, not on a pass over the frame
        if y.dtype.kind in "biu" or np.all(y == np.floor(y)):
            yi = np.asarray(y, dtype=np.int64)
            if ((yi == 0) | (yi == 1)).all():
                return yi.astype(np.uint8), None
            ok = (self.code.syndrome(yi) == 0).all(axis=-1)  # integer-valued, not binary: decide on the host
            return None, np.atleast_1d(ok)
        return None, None

    def decode(self, y, priors):
        y = np.asarray(y)
        y0, host_ok = self._iter0_word(y)
        if host_ok is not None and host_ok[0]:  # passes the iteration-0 test of src/bpa.py:28-29 for every max_iter (0 included)
            self.last_iters = np.zeros(1, dtype=np.int32)
            return y
        xhat, iters = self.handle.decode_host(np.asarray(priors), y0, self.max_iter)
        self.last_iters = iters
        if iters[0] == 0 and y0 is not None:
            return y  # left at the iteration-0 check: upstream returns the received object itself
        return xhat[0].astype(np.int64)

    def decode_batch(self, y, priors):
        """[B,n] frames -> (x_hat uint8 [B,n], iters int32 [B]).  numpy in -> numpy out; CUDA tensors in -> CUDA
        tensors out (no copies; y may be None or a uint8 tensor of hard received words)."""
        if hasattr(priors, "is_cuda"):
            out = self.handle.decode_device(priors, y, self.max_iter)
            self.last_iters = out[1]
            return out
        y0 = None
        if y is not None:
            y0, host_ok = self._iter0_word(y)
            if host_ok is not None and host_ok.any():
                raise ValueError("integer-valued non-binary received words are only supported one frame at a time")
        out = self.handle.decode_host(priors, y0, self.max_iter)
        self.last_iters = out[1]
        return out


class SPA(BPA):
    """Sum-product: tanh-product check rule (src/bpa.py:66-75)."""
    alg = "SPA"


class MSA(BPA):
    """Min-sum: two-min + sign-parity check rule (src/bpa.py:78-102)."""
    alg = "MSA"


class NMSA(BPA):
    """Corrected min-sum (no upstream counterpart): the rule of src/bpa.py:86-102 with every check message scaled and / or offset,
    ``c2v = sign * max(msa_scale * min - msa_offset, 0)`` -- normalised min-sum (0 < msa_scale <= 1), offset min-sum (msa_offset >= 0) or
    both.  (1, 0) is ``MSA`` bit for bit.  Same ``decode`` / ``decode_batch``, kernels, shapes and precisions as ``MSA``."""
    alg = "NMSA"
    id_keys = ["max_iter", "msa_scale", "msa_offset"]

    def __init__(self, parity_mtx, **kwargs):
        scale = kwargs.get("msa_scale")
        offset = kwargs.get("msa_offset")
        # (checked before the decoder is created: a bad value never reaches the device)
        self.msa_scale, self.msa_offset = check_correction(0.8125 if scale is None else scale, 0.0 if offset is None else offset)
        super().__init__(parity_mtx, **kwargs)
        self.handle.set_correction(self.msa_scale, self.msa_offset)


class LMSA(BPA):
    """Layered (serial-C) corrected min-sum (no upstream counterpart): the check rule of ``NMSA``, but the checks are processed layer by
    layer and every layer already sees the marginals the one before it left -- about half the sweeps of the flooding schedule.  ``layers``:
    the layer of every check (two checks of a layer share no variable); None: greedy, every check takes the first layer it fits.  Runs on
    the streaming kernels in f32 / f64; ``decode`` / ``decode_batch`` as ``NMSA``.  The contract: include/ldpc_hip.h (LDPC_ALG_LMSA)."""
    alg = "LMSA"
    id_keys = ["max_iter", "msa_scale", "msa_offset"]

    def __init__(self, parity_mtx, **kwargs):
        scale, offset, layers = kwargs.get("msa_scale"), kwargs.get("msa_offset"), kwargs.get("layers")
        # (checked before the decoder is created: a bad value never reaches the device)
        self.msa_scale, self.msa_offset = check_correction(0.8125 if scale is None else scale, 0.0 if offset is None else offset)
        code = as_code(parity_mtx)
        if layers is not None:
            layers = check_layers(code, layers)
        if np.bincount(np.asarray(code.edge_chk), minlength=code.m).min() < 2:
            raise ValueError("layered min-sum needs every check to have at least two variables")
        if kwargs.get("precision") == "f16" or kwargs.get("backend") == "fused":
            raise ValueError("layered min-sum runs on the streaming kernels in f32 or f64")
        super().__init__(code, **kwargs)
        self.handle.set_correction(self.msa_scale, self.msa_offset)
        if layers is not None:
            self.handle.set_layers(layers)

    @property
    def layers(self):
        """The layer of every check, as the library holds it (``ldpc_decoder_get_layers``)."""
        return self.handle.layers()[1]


class QMSA(BPA):
    """Fixed-point min-sum (no upstream counterpart): the decoder as silicon builds it.  Priors are quantised to ``msa_bits``-bit levels,
    ``clamp(rint(prior * 2**msa_frac_bits), -V, V)`` with ``V = 2**(msa_bits - 1) - 1``; every check message is
    ``sign * max(floor(msa_scale * min(m, V)) - msa_offset, 0)`` (``msa_scale`` on the 1/64 grid, ``msa_offset`` an integer number of levels).
    All values are small integers: every precision and backend returns the same decisions and iteration counts, those of an all-integer
    model.  Same ``decode`` / ``decode_batch``, kernels and shapes as ``MSA``; soft outputs are in levels."""
    alg = "QMSA"
    id_keys = ["max_iter", "msa_bits", "msa_frac_bits", "msa_scale", "msa_offset"]

    def __init__(self, parity_mtx, **kwargs):
        given = [kwargs.get(k) for k in ("msa_bits", "msa_frac_bits", "msa_scale", "msa_offset")]
        values = [d if v is None else v for v, d in zip(given, (6, 2, 0.8125, 0))]
        # (checked before the decoder is created: a bad value never reaches the device)
        self.msa_bits, self.msa_frac_bits, self.msa_scale, self.msa_offset = check_fixed_point(*values)
        super().__init__(parity_mtx, **kwargs)
        self.handle.set_fixed_point(self.msa_bits, self.msa_frac_bits, self.msa_scale, self.msa_offset)


OSD_LDS_BYTES = 160 * 1024  # one CU's LDS: a frame's sort keys, matrix and permutations must fit
OSD_MAX_ROWS = 4096


def osd_lds_bytes(m, n):
    """LDS one frame of the ordered-statistics post-processor takes: the rule of ldpc_osd_create (osd_lds_words, csrc/ldpc_osd.hpp)."""
    NP, S, RP = 1, (n + 31) // 32, -(-m // 64) * 64
    while NP < n:
        NP <<= 1
    return 4 * (2 * NP + S * RP + 4 * n + 5 * S)


def check_osd_size(code):
    """ValueError unless a frame of ``code`` fits one CU's LDS (checked before the library is loaded)."""
    if osd_lds_bytes(code.m, code.n) > OSD_LDS_BYTES or -(-code.m // 64) * 64 > OSD_MAX_ROWS:
        raise ValueError("ordered-statistics post-processing: a frame of a %d x %d code needs %d bytes of LDS (sort keys, matrix, "
                         "permutations), above the limit of one CU's 160 KiB (at most %d checks)"
                         % (code.m, code.n, osd_lds_bytes(code.m, code.n), OSD_MAX_ROWS))


class OSD:
    """Belief propagation followed by ordered-statistics decoding of the frames it leaves without a codeword (no upstream counterpart; it
    adds to ``BPA.decode``, src/bpa.py:17-63).  ``osd_bp`` in {MSA, SPA, NMSA, QMSA, LMSA} names the decoder in front (its own keywords apply),
    ``osd_order`` in {0, 1}, ``osd_depth`` >= 0 the number of single flips order 1 tries.  The output is always a codeword.  ``decode`` /
    ``decode_batch`` as ``BPA``; ``last_pick`` holds per frame -1 (BP's word, untouched) or the winning candidate.  The contract:
    include/ldpc_hip.h (ldpc_osd_*), DESIGN.md section 17."""
    id_keys = ["max_iter", "msa_scale", "msa_offset", "osd_order", "osd_depth"]

    def __init__(self, parity_mtx, **kwargs):
        self.max_iter = kwargs["max_iter"]
        self.code = as_code(parity_mtx)
        check_osd_size(self.code)
        order, depth = kwargs.get("osd_order"), kwargs.get("osd_depth")
        self.osd_order, self.osd_depth = 0 if order is None else int(order), 64 if depth is None else int(depth)
        if self.osd_order not in (0, 1) or self.osd_depth < 0:
            raise ValueError("osd_order must be 0 or 1 and osd_depth >= 0 (got %r, %r)" % (order, depth))
        self.osd_bp = kwargs.get("osd_bp") or "NMSA"
        from .registry import osd_fronts  # (here: the registry imports this module)

        front = osd_fronts().get(self.osd_bp)
        if front is None:
            raise ValueError("osd_bp must be one of %s (got %r)" % (", ".join(osd_fronts()), self.osd_bp))
        self.precision = kwargs.get("precision") or "f64"
        if self.precision not in ("f32", "f64"):
            raise ValueError("ordered-statistics post-processing needs the soft output of an f32 or f64 decoder (got precision %r)" % self.precision)
        # (every keyword goes on to the decoder in front.  ``layers`` then means a layering of the checks to LMSA: a caller that forwards
        # command-line arguments must drop the ADMMA flag of that name first, as main.py does)
        self.bp = front(self.code, **kwargs)
        self.handle = OsdHandle(self.bp.handle, self.osd_order, self.osd_depth)
        self.last_iters = self.last_pick = None

    @property
    def parity_mtx(self):
        return self.code.parity_mtx

    def _host(self, y0, priors):
        import torch

        dev = "cuda:%d" % self.handle.device
        pri = torch.from_numpy(np.ascontiguousarray(np.atleast_2d(priors), dtype=self.bp.handle.np_dtype)).to(dev)
        if pri.shape[1] != self.code.n:
            raise ValueError("frames must have n=%d entries" % self.code.n)
        yd = None if y0 is None else torch.from_numpy(np.ascontiguousarray(np.atleast_2d(y0), dtype=np.uint8)).to(dev)
        xhat, iters, pick = self.handle.decode_device(pri, yd, self.max_iter)
        return xhat.cpu().numpy(), iters.cpu().numpy(), pick.cpu().numpy()

    def decode(self, y, priors):
        y = np.asarray(y)
        y0, host_ok = self.bp._iter0_word(y)
        if host_ok is not None and host_ok[0]:  # passes the iteration-0 test of src/bpa.py:28-29: the received word is a codeword
            self.last_iters, self.last_pick = np.zeros(1, dtype=np.int32), np.full(1, -1, dtype=np.int32)
            return y
        xhat, self.last_iters, self.last_pick = self._host(y0, np.asarray(priors))
        if self.last_iters[0] == 0 and y0 is not None:
            return y  # left at the iteration-0 check: upstream returns the received object itself
        return xhat[0].astype(np.int64)

    def decode_batch(self, y, priors):
        """[B,n] frames -> (x_hat uint8 [B,n], BP's iters int32 [B]).  numpy in -> numpy out; CUDA tensors in -> CUDA tensors out."""
        if hasattr(priors, "is_cuda"):
            xhat, self.last_iters, self.last_pick = self.handle.decode_device(priors, y, self.max_iter)
            return xhat, self.last_iters
        y0 = None
        if y is not None:
            y0, host_ok = self.bp._iter0_word(y)
            if host_ok is not None and host_ok.any():
                raise ValueError("integer-valued non-binary received words are only supported one frame at a time")
        xhat, self.last_iters, self.last_pick = self._host(y0, priors)
        return xhat, self.last_iters
