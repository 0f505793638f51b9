"""Layered fixed-point min-sum, LDS-resident (``LQMSA``) and on the streaming kernels (``SLQMSA``) (no upstream counterpart -- ``BPA.decode``, src/bpa.py:17-63, runs the flooding schedule in
floating point).  ``QMSA``'s integer rule on ``LMSA``'s schedule with the whole frame in the LDS as integers: int16 marginals, int8 check
messages.  The contract is the ``ldpc_lqmsa_*`` block of include/ldpc_hip.h;
``SLQMSA`` keeps the same integers in HBM tiles for the codes whose frame does not fit the LDS (``ldpc_slq_*``)."""
import numpy as np

from ._device import LqmsaHandle, SlqHandle, as_code, check_layers

LDS_BYTES = 160 * 1024
MAX_DV = 255


def lqmsa_row_bytes(dc_max):
    """Bytes of one check's row of int8 messages (csrc/ldpc_lqmsa.hpp lqmsa_row_bytes): 8 up to degree 8, whole dwords above it."""
    return 8 if dc_max <= 8 else (dc_max + 3) // 4 * 4


def lqmsa_lds_bytes(m, n, E, dc_max):
    """LDS bytes one frame takes in the kernel (csrc/ldpc_lqmsa.hpp lqmsa_lds_bytes): the int16 marginals rounded up to 8 bytes, one
    message row per check, 16 bytes of frame state; ``E`` does not enter this layout.  A frame fits iff this is at most ``LDS_BYTES``."""
    return (2 * n + 7) // 8 * 8 + m * lqmsa_row_bytes(dc_max) + 16


def lqmsa_waves(frames_per_cu):
    """Waves per frame (csrc/ldpc_lqmsa.hpp lqmsa_waves): the CU is to hold as many waves as it can, up to 32 -- min(frames, 32 // W) * W --
    with the smallest W of 1, 2, 4, 8 that reaches the most."""
    return max((1, 2, 4, 8), key=lambda w: (min(frames_per_cu, 32 // w) * w, -w))


def check_params(bits, frac_bits, scale, offset):
    """What ``ldpc_lqmsa_set_fixed_point`` accepts -- 2 <= bits <= 8, -8 <= frac_bits <= 8, scale a multiple of 1/64 in (0, 1], an integer
    offset >= 0 (in levels) -- checked before any device call.  -> (bits, frac_bits, scale, offset) as int, int, float, int."""
    scale, off = float(scale), float(offset)
    ok = float(bits) == int(bits) and float(frac_bits) == int(frac_bits) and 2 <= int(bits) <= 8 and -8 <= int(frac_bits) <= 8
    ok = ok and 0.0 < scale <= 1.0 and scale * 64.0 == int(scale * 64.0) and 0.0 <= off < float("inf") and off == int(off)
    if not ok:
        raise ValueError("layered fixed-point min-sum needs 2 <= bits <= 8, -8 <= frac_bits <= 8, a scale on the 1/64 grid with 0 < scale <= 1 "
                         "and an integer offset >= 0 (got bits=%r, frac_bits=%r, scale=%r, offset=%r)" % (bits, frac_bits, scale, offset))
    return int(bits), int(frac_bits), scale, int(off)


def check_code(code):
    """ValueError unless ``ldpc_lqmsa_create`` takes the code (checked before the library is loaded)."""
    dc = np.bincount(np.asarray(code.edge_chk), minlength=code.m)
    dv = np.bincount(np.asarray(code.edge_var), minlength=code.n)
    if dc.min() < 2:
        raise ValueError("layered min-sum needs every check to have at least two variables")
    if dv.max() > MAX_DV:
        raise ValueError("LQMSA: a variable of degree %d: the int16 marginals hold degrees up to %d" % (dv.max(), MAX_DV))
    need = lqmsa_lds_bytes(code.m, code.n, code.E, int(dc.max()))
    if need > LDS_BYTES or code.n > 65536:
        raise ValueError("LQMSA: a frame of a %d x %d code (largest check degree %d) needs %d bytes of LDS, above one CU's %d; "
                         "use LMSA (layered min-sum on the streaming kernels) for it" % (code.m, code.n, dc.max(), need, LDS_BYTES))


class LQMSA:
    """Layered fixed-point min-sum.  Priors are quantised to ``msa_bits``-bit levels as ``QMSA`` does, the checks are processed layer by
    layer as ``LMSA`` does (``layers``: the layer of every check, None: greedy), every check message is
    ``sign * max((64 msa_scale * min(m, V)) >> 6 - msa_offset, 0)``.  ``decode(y, priors)`` / ``decode_batch(y, priors)`` as ``bpa.BPA``:
    numpy in -> numpy out, CUDA tensors in -> CUDA tensors out; ``last_iters`` holds the sweeps of the last call."""
    id_keys = ["max_iter", "msa_bits", "msa_frac_bits", "msa_scale", "msa_offset"]

    def __init__(self, parity_mtx, max_iter=10, msa_bits=6, msa_frac_bits=2, msa_scale=0.8125, msa_offset=0, layers=None, **_):
        given = (msa_bits, msa_frac_bits, msa_scale, msa_offset)
        values = [d if v is None else v for v, d in zip(given, (6, 2, 0.8125, 0))]
        # (checked before the decoder is created: a bad value never reaches the device)
        self.msa_bits, self.msa_frac_bits, self.msa_scale, self.msa_offset = check_params(*values)
        if _.get("precision") == "f16" or _.get("backend") == "stream":
            raise ValueError("LQMSA is an LDS-resident integer kernel: no fp16 storage, no streaming backend (LMSA has one)")
        self.max_iter = int(max_iter)
        self.code = as_code(parity_mtx)
        if layers is not None:
            layers = check_layers(self.code, layers)
        check_code(self.code)
        self.precision = "f64" if _.get("precision") == "f64" else "f32"  # the type the priors are quantised in
        self.handle = LqmsaHandle(self.code, _.get("device"), self.msa_bits, self.msa_frac_bits, self.msa_scale, self.msa_offset)
        if layers is not None:
            self.handle.set_layers(layers)
        self.last_iters = None

    @property
    def parity_mtx(self):
        return self.code.parity_mtx

    @property
    def layers(self):
        """The layer of every check, as the library holds it (``ldpc_lqmsa_get_layers``)."""
        return self.handle.layers()[1]

    def _host(self, y, priors):
        import torch

        priors = np.ascontiguousarray(np.atleast_2d(priors), dtype=np.float64 if self.precision == "f64" else np.float32)
        if priors.ndim != 2 or priors.shape[1] != self.code.n:
            raise ValueError("frames must have n=%d entries" % self.code.n)
        dev = "cuda:%d" % self.handle.device
        y0 = None
        if y is not None:
            y = np.atleast_2d(np.asarray(y))
            if y.dtype.kind in "biu" and ((y == 0) | (y == 1)).all():  # a hard received word takes the iteration-0 check (src/bpa.py:20,29)
                y0 = torch.from_numpy(np.ascontiguousarray(y, dtype=np.uint8)).to(dev)
        xhat, iters = self.handle.decode_device(torch.from_numpy(priors).to(dev), y0, self.max_iter)
        return xhat.cpu().numpy(), iters.cpu().numpy()

    def decode(self, y, priors):
        xhat, self.last_iters = self._host(y, np.asarray(priors))
        return xhat[0].astype(np.int64)

    def decode_batch(self, y, priors):
        """[B, n] frames -> (x_hat uint8 [B, n], iters int32 [B]); ``y`` may be None or the hard received words."""
        if hasattr(priors, "is_cuda"):
            out = self.handle.decode_device(priors, y, self.max_iter)
        else:
            out = self._host(y, priors)
        self.last_iters = out[1]
        return out


def check_code_streamed(code):
    """ValueError unless ``ldpc_slq_create`` takes the code (checked before the library is loaded): the two degree rules of ``check_code``
    and no size rule."""
    dc = np.bincount(np.asarray(code.edge_chk), minlength=code.m)
    dv = np.bincount(np.asarray(code.edge_var), minlength=code.n)
    if dc.min() < 2:
        raise ValueError("layered min-sum needs every check to have at least two variables")
    if dv.max() > MAX_DV:
        raise ValueError("SLQMSA: a variable of degree %d: the int16 marginals hold degrees up to %d" % (dv.max(), MAX_DV))


class SLQMSA(LQMSA):
    """Layered fixed-point min-sum on the streaming kernels: ``LQMSA``'s rule, parameters, layers and outputs, bit for bit, with the int16
    marginals and int8 messages in HBM tiles instead of the LDS -- any code, whatever its size.  ``decode`` / ``decode_batch`` / ``layers``
    / ``last_iters`` as ``LQMSA``."""

    def __init__(self, parity_mtx, max_iter=10, msa_bits=6, msa_frac_bits=2, msa_scale=0.8125, msa_offset=0, layers=None, **_):
        given = (msa_bits, msa_frac_bits, msa_scale, msa_offset)
        values = [d if v is None else v for v, d in zip(given, (6, 2, 0.8125, 0))]
        # (checked before the decoder is created: a bad value never reaches the device)
        self.msa_bits, self.msa_frac_bits, self.msa_scale, self.msa_offset = check_params(*values)
        if _.get("precision") == "f16" or _.get("backend") == "fused":
            raise ValueError("SLQMSA keeps integer tiles in HBM: no fp16 storage, no LDS-resident backend (LQMSA is the LDS-resident kernel)")
        self.max_iter = int(max_iter)
        self.code = as_code(parity_mtx)
        if layers is not None:
            layers = check_layers(self.code, layers)
        check_code_streamed(self.code)
        self.precision = "f64" if _.get("precision") == "f64" else "f32"  # the type the priors are quantised in
        self.handle = SlqHandle(self.code, _.get("device"), self.msa_bits, self.msa_frac_bits, self.msa_scale, self.msa_offset)
        if layers is not None:
            self.handle.set_layers(layers)
        self.last_iters = None
