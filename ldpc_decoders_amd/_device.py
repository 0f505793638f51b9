"""Device-side handles: Tanner graph in HBM and decoder workspaces (thin wrappers over the C ABI)."""
import ctypes

import numpy as np

from . import _lib
from .codes import Code


def as_code(obj):
    """Accept a ``codes.Code`` or a dense parity matrix (the reference passes ``code.parity_mtx``, src/biawgn.py:35)."""
    if isinstance(obj, Code):
        return obj
    if hasattr(obj, "edge_chk") and hasattr(obj, "edge_var"):
        return Code.from_edges(obj.m, obj.n, obj.edge_chk, obj.edge_var)
    return Code(None, np.asarray(obj))


def current_device():
    try:
        import torch

        if torch.cuda.is_available():
            return torch.cuda.current_device()
    except ImportError:
        pass
    return 0


def unpack_bits(bits, n, erased=None):
    """Packed decisions (uint32 / int32 words, numpy) -> bytes [B,n] in {0,1} ({0,1,2} with the erased mask), as ldpc_decode returns them."""
    words = np.ascontiguousarray(bits).view(np.uint8)
    x = np.unpackbits(words, axis=1, bitorder="little")[:, :n]
    if erased is not None:
        e = np.unpackbits(np.ascontiguousarray(erased).view(np.uint8), axis=1, bitorder="little")[:, :n]
        x = np.where(e == 1, np.uint8(2), x)
    return x


def check_correction(scale, offset):
    """The range ``ldpc_decoder_set_correction`` accepts (0 < scale <= 1, finite offset >= 0), checked before any device call."""
    scale, offset = float(scale), float(offset)
    if not (0.0 < scale <= 1.0) or not (0.0 <= offset < float("inf")):
        raise ValueError("corrected min-sum needs 0 < scale <= 1 and a finite offset >= 0 (got scale=%r, offset=%r)" % (scale, offset))
    return scale, offset


def check_fixed_point(bits, frac_bits, scale, offset):
    """The range ``ldpc_decoder_set_fixed_point`` accepts -- 2 <= bits <= 12, -8 <= frac_bits <= 8, scale a multiple of 1/64 in (0, 1], an
    integer offset >= 0 (in levels) -- checked before any device call.  -> (bits, frac_bits, scale, offset) as int, int, float, int."""
    scale, off = float(scale), float(offset)
    ok = float(bits) == int(bits) and float(frac_bits) == int(frac_bits) and 2 <= int(bits) <= 12 and -8 <= int(frac_bits) <= 8
    ok = ok and 0.0 < scale <= 1.0 and scale * 64.0 == int(scale * 64.0) and 0.0 <= off < float("inf") and off == int(off)
    if not ok:
        raise ValueError("fixed-point min-sum needs 2 <= bits <= 12, -8 <= frac_bits <= 8, a scale on the 1/64 grid with 0 < scale <= 1 and an "
                         "integer offset >= 0 (got bits=%r, frac_bits=%r, scale=%r, offset=%r)" % (bits, frac_bits, scale, offset))
    return int(bits), int(frac_bits), scale, int(off)


def check_layers(code, layers):
    """What ``ldpc_decoder_set_layers`` accepts -- one non-negative integer per check, no two checks of a layer on one variable -- checked
    before any device call.  -> the layering as an int64 array."""
    lay = np.asarray(layers)
    if lay.ndim != 1 or lay.size != code.m or lay.dtype.kind not in "iu" or (lay < 0).any() or (lay >= 2 ** 31).any():
        raise ValueError("a layering is one non-negative integer per check (%d checks)" % code.m)
    lay = lay.astype(np.int64)
    key = np.asarray(code.edge_var, dtype=np.int64) * (int(lay.max()) + 1) + lay[np.asarray(code.edge_chk)]
    if np.unique(key).size != key.size:
        raise ValueError("two checks of one layer share a variable")
    return lay


class FamilyHandle:
    """A handle of one ``<family>_*`` block of the C ABI: ``h`` is made by ``<family>_create(*args, &h)`` and given back to
    ``<family>_destroy`` with the object; ``_fn(name)`` is the library's ``<family>_<name>``."""
    family = None

    def _fn(self, name):
        return getattr(_lib.load(), "%s_%s" % (self.family, name))

    def _create(self, *args):
        h = ctypes.c_void_p()
        _lib.check(self._fn("create")(*args, ctypes.byref(h)))
        self.h = h

    def _create_on_code(self, code, device, *args):
        """``_create`` for a family that lives on a code: ``<family>_create(code handle, *args, &h)``; sets code_handle, code and device."""
        self.code_handle = code_handle(code, device)
        self.code, self.device = code, self.code_handle.device
        self._create(self.code_handle.h, *args)

    def __del__(self):
        try:
            if getattr(self, "h", None):
                self._fn("destroy")(self.h)
                self.h = None
        except Exception:
            pass


class FixedPointLayers:
    """The fixed-point parameters and the layering of a ``FamilyHandle`` whose family has ``set/get_fixed_point`` and ``set/get_layers``
    (``ldpc_decoder``, ``ldpc_lqmsa``, ``ldpc_slq``; ``ldpc_qc`` has the first pair).  Handle state, in force from the next call; the
    library refuses what is out of range with an ``LdpcHipError`` that names the entry point."""

    def set_fixed_point(self, bits, frac_bits, scale, offset=0):
        _lib.check(self._fn("set_fixed_point")(self.h, int(bits), int(frac_bits), float(scale), int(offset)))

    def fixed_point(self):
        b, k, o, s = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0), ctypes.c_double(0)
        _lib.check(self._fn("get_fixed_point")(self.h, ctypes.byref(b), ctypes.byref(k), ctypes.byref(s), ctypes.byref(o)))
        return b.value, k.value, s.value, o.value

    def set_layers(self, layers=None):
        """``layers``: one non-negative int per check (two checks of one layer share no variable), or None for the greedy layering."""
        if layers is None:
            _lib.check(self._fn("set_layers")(self.h, None, 0))
            return
        lay = np.ascontiguousarray(check_layers(self.code, layers), dtype=np.int32)
        _lib.check(self._fn("set_layers")(self.h, lay.ctypes.data, lay.size))

    def layers(self):
        """-> (number of layers, layer of every check as int32 [m])"""
        nl, lay = ctypes.c_int32(0), np.empty(self.code.m, dtype=np.int32)
        _lib.check(self._fn("get_layers")(self.h, ctypes.byref(nl), lay.ctypes.data))
        return nl.value, lay


def channel_sent(channel, precision, param, sent, seed, stream_id, frame0, priors=True):
    """``ldpc_channel_sent``: the channel of ``DecoderHandle.channel_device`` for the given words ``sent`` (CUDA uint8 [B, n]), one per frame
    of [frame0, frame0 + B).  -> (priors in ``precision`` or None, y or None); ``priors=False`` asks for the received word alone."""
    import torch

    B, n = sent.shape
    dt = torch.float64 if precision == "f64" else torch.float32
    pri = torch.empty((B, n), dtype=dt, device=sent.device) if priors and channel != "bec" else None
    y = None if channel == "biawgn" else torch.empty((B, n), dtype=torch.uint8, device=sent.device)
    st = torch.cuda.current_stream(sent.device).cuda_stream
    _lib.check(_lib.load().ldpc_channel_sent(_lib.CHANNEL[channel], _lib.IO_DTYPE[precision], float(param), sent.data_ptr(), int(seed),
                                             int(stream_id), int(frame0), B, n, None if pri is None else pri.data_ptr(),
                                             None if y is None else y.data_ptr(), st))
    return pri, y


def channel_pattern(channel, precision, param, sent, codeword, kind, short_llr, seed, stream_id, frame0, B=None):
    """``ldpc_channel_pattern``: the channel of ``channel_sent`` under a transmission pattern, ``kind`` CUDA uint8 [n] (0 sent, 1 punctured:
    prior +0.0, 2 shortened: prior +short_llr).  ``sent`` CUDA uint8 [B, n], or None for ``B`` frames of the all-``codeword`` word.
    -> (priors in ``precision``, y or None)"""
    import torch

    n = kind.shape[0]
    B = int(B) if sent is None else sent.shape[0]
    dt = torch.float64 if precision == "f64" else torch.float32
    pri = torch.empty((B, n), dtype=dt, device=kind.device)
    y = None if channel == "biawgn" else torch.empty((B, n), dtype=torch.uint8, device=kind.device)
    st = torch.cuda.current_stream(kind.device).cuda_stream
    _lib.check(_lib.load().ldpc_channel_pattern(_lib.CHANNEL[channel], _lib.IO_DTYPE[precision], float(param), None if sent is None else sent.data_ptr(),
                                                int(codeword), kind.data_ptr(), float(short_llr), int(seed), int(stream_id), int(frame0), B, n,
                                                pri.data_ptr(), None if y is None else y.data_ptr(), st))
    return pri, y


def decode_drawn(handle, draw, max_iter, flags):
    """The decode of given words, stated once for every LLR handle class (``DecoderHandle``, ``OsdHandle``, ``LqmsaHandle`` and its
    subclasses): -> ``decode(sent, first frame)`` -> (xhat, iters), which asks ``draw(precision, sent, first)`` -- ``channel_sent``, or
    ``channel_pattern`` under a transmission pattern -- for (priors, y) in the handle's precision and hands them to its ``decode_device``."""
    def decode(sent, first):
        pri, y = draw(handle.precision, sent, first)
        return handle.decode_device(pri, y, max_iter, flags)[:2]

    return decode


def draw_sent(channel, param, seed, stream_id):
    """The ``draw`` of ``decode_drawn`` without a pattern: ``channel_sent`` of the words."""
    return lambda precision, sent, first: channel_sent(channel, precision, param, sent, seed, stream_id, first)


def simulate_random_codewords(code, device, seed, stream_id, frame0, B, chunk, counters, hist_bins, decode):
    """``codeword == -1`` for a code without a code book, stated once for every handle class: frames [frame0, frame0 + B) in chunks of
    ``chunk`` (the class's ``words_chunk``), each a random codeword from the systematic encoder (``Code.encoder()``) ->
    ``decode(sent, first frame of the chunk)`` -> (xhat uint8 [nb, n], iters or None), which sends the words through ``channel_sent`` and
    decodes them -> counted against the sent words into ``counters``."""
    import torch

    lib, n = _lib.load(), code.n
    enc = code.encoder().handle(device)
    st = torch.cuda.current_stream(counters.device).cuda_stream
    for b0 in range(0, int(B), int(chunk)):
        nb = min(int(chunk), int(B) - b0)
        sent = enc.encode_random(seed, stream_id, int(frame0) + b0, nb)
        xhat, iters = decode(sent, int(frame0) + b0)
        _lib.check(lib.ldpc_count_errors_words(xhat.data_ptr(), sent.data_ptr(), None if iters is None else iters.data_ptr(), nb, n, hist_bins,
                                               counters.data_ptr(), st))


class CodeHandle(FamilyHandle):
    family = "ldpc_code"

    def __init__(self, code, device):
        self.code, self.device = code, device
        chk = np.ascontiguousarray(code.edge_chk, dtype=np.int32)
        var = np.ascontiguousarray(code.edge_var, dtype=np.int32)
        self._create(device, code.m, code.n, code.E, chk.ctypes.data, var.ctypes.data)


def code_handle(code, device=None):
    device = current_device() if device is None else device
    hd = code._handles.get(device)
    if hd is None:
        hd = code._handles[device] = CodeHandle(code, device)
    return hd


class DecoderHandle(FixedPointLayers, FamilyHandle):
    """One (graph, algorithm, arithmetic, backend) decoder with its HBM workspace."""
    family = "ldpc_decoder"

    def __init__(self, code, alg, precision="f32", backend="auto", device=None):
        self.code_handle = code_handle(code, device)
        self.code, self.alg, self.precision, self.backend = code, alg, precision, backend
        self.np_dtype = np.float64 if precision == "f64" else np.float32
        self._create(self.code_handle.h, _lib.ALG[alg], _lib.DTYPE[precision], _lib.BACKEND[backend])

    # ---- corrected min-sum (alg="NMSA"): c2v = sign * max(scale * min - offset, 0); decoder state, in force from the next call
    def set_correction(self, scale, offset=0.0):
        check_correction(scale, offset)
        _lib.check(_lib.load().ldpc_decoder_set_correction(self.h, float(scale), float(offset)))

    def correction(self):
        s, o = ctypes.c_double(0), ctypes.c_double(0)
        _lib.check(_lib.load().ldpc_decoder_get_correction(self.h, ctypes.byref(s), ctypes.byref(o)))
        return s.value, o.value

    # ---- fixed-point min-sum (alg="QMSA"): q-bit levels, c2v = sign * max(floor(scale * min(m, V)) - offset, 0); decoder state, in force
    # from the next call (``fixed_point()`` reads it back); checked here first, so what is out of range raises ValueError
    def set_fixed_point(self, bits, frac_bits, scale, offset=0):
        super().set_fixed_point(*check_fixed_point(bits, frac_bits, scale, offset))

    # ---- layered min-sum (alg="LMSA"): the layer of every check, ``set_layers`` / ``layers`` of FixedPointLayers

    # ---- host (numpy) buffers
    def decode_host(self, priors, y0, max_iter, flags=0):
        lib = _lib.load()
        n = self.code.n
        if self.alg == "BEC":
            y0 = np.ascontiguousarray(np.atleast_2d(y0), dtype=np.uint8)
            B, pri_ptr = y0.shape[0], None
        else:
            priors = np.ascontiguousarray(np.atleast_2d(priors), dtype=self.np_dtype)
            B, pri_ptr = priors.shape[0], priors.ctypes.data
            if y0 is not None:
                y0 = np.ascontiguousarray(np.atleast_2d(y0), dtype=np.uint8)
        if (priors is not None and self.alg != "BEC" and priors.shape[1] != n) or (y0 is not None and y0.shape[1] != n):
            raise ValueError("frames must have n=%d entries" % n)
        xhat = np.empty((B, n), dtype=np.uint8)
        iters = np.empty(B, dtype=np.int32)
        _lib.check(lib.ldpc_decode_host(self.h, pri_ptr, None if y0 is None else y0.ctypes.data, B, int(max_iter), flags,
                                        xhat.ctypes.data, iters.ctypes.data))
        return xhat, iters

    # ---- device (torch) buffers: no copies, current torch stream
    def decode_device(self, priors, y0, max_iter, flags=0, xhat=None, iters=None):
        import torch

        lib = _lib.load()
        n = self.code.n
        ref = y0 if priors is None else priors
        B = ref.shape[0]
        if priors is not None:
            want = torch.float64 if self.precision == "f64" else torch.float32
            if priors.dtype != want or not priors.is_contiguous() or not priors.is_cuda:
                raise ValueError("priors must be a contiguous CUDA tensor of dtype %s" % want)
        if y0 is not None and (y0.dtype != torch.uint8 or not y0.is_contiguous() or not y0.is_cuda):
            raise ValueError("y0 must be a contiguous CUDA uint8 tensor")
        if xhat is None:
            xhat = torch.empty((B, n), dtype=torch.uint8, device=ref.device)
        if iters is None:
            iters = torch.empty((B,), dtype=torch.int32, device=ref.device)
        if B == 0:
            return xhat, iters
        st = torch.cuda.current_stream(ref.device).cuda_stream
        _lib.check(lib.ldpc_decode(self.h, None if priors is None else priors.data_ptr(), None if y0 is None else y0.data_ptr(),
                                   B, int(max_iter), flags, xhat.data_ptr(), iters.data_ptr(), st))
        return xhat, iters

    def decode_device_bits(self, priors, y0, max_iter, flags=0):
        """``ldpc_decode_bits``: packed decisions.  -> (xhat_bits int32 [B, ceil(n/32)] viewed as uint32 words, erased_bits or None, iters);
        bit (v & 31) of word (v >> 5) = decision of variable v.  ``unpack_bits`` expands them."""
        import torch

        ref = y0 if priors is None else priors
        B, W = ref.shape[0], (self.code.n + 31) // 32
        bits = torch.empty((B, W), dtype=torch.int32, device=ref.device)
        era = torch.empty((B, W), dtype=torch.int32, device=ref.device) if self.alg == "BEC" else None
        iters = torch.empty((B,), dtype=torch.int32, device=ref.device)
        if B == 0:
            return bits, era, iters
        st = torch.cuda.current_stream(ref.device).cuda_stream
        _lib.check(_lib.load().ldpc_decode_bits(self.h, None if priors is None else priors.data_ptr(), None if y0 is None else y0.data_ptr(),
                                                B, int(max_iter), flags, bits.data_ptr(), None if era is None else era.data_ptr(),
                                                iters.data_ptr(), st))
        return bits, era, iters

    def decode_host_bits(self, priors, y0, max_iter, flags=0):
        """``ldpc_decode_host_bits``: numpy in, packed decisions out -> (xhat_bits uint32 [B,W], erased_bits uint32 [B,W] or None, iters)."""
        n = self.code.n
        W = (n + 31) // 32
        if self.alg == "BEC":
            y0 = np.ascontiguousarray(np.atleast_2d(y0), dtype=np.uint8)
            B, pri_ptr = y0.shape[0], None
        else:
            priors = np.ascontiguousarray(np.atleast_2d(priors), dtype=self.np_dtype)
            B, pri_ptr = priors.shape[0], priors.ctypes.data
            if y0 is not None:
                y0 = np.ascontiguousarray(np.atleast_2d(y0), dtype=np.uint8)
        bits = np.zeros((B, W), dtype=np.uint32)
        era = np.zeros((B, W), dtype=np.uint32) if self.alg == "BEC" else None
        iters = np.empty(B, dtype=np.int32)
        _lib.check(_lib.load().ldpc_decode_host_bits(self.h, pri_ptr, None if y0 is None else y0.ctypes.data, B, int(max_iter), flags,
                                                     bits.ctypes.data, None if era is None else era.ctypes.data, iters.ctypes.data))
        return bits, era, iters

    def count_errors_bits(self, bits, era, iters, counters, codeword=0, hist_bins=0):
        import torch

        st = torch.cuda.current_stream(counters.device).cuda_stream
        _lib.check(_lib.load().ldpc_count_errors_bits(bits.data_ptr(), None if era is None else era.data_ptr(), None, int(codeword),
                                                      None if iters is None else iters.data_ptr(), bits.shape[0], self.code.n, hist_bins,
                                                      counters.data_ptr(), st))

    def decode_soft_device(self, priors, y0, max_iter, flags=0):
        """Streaming backend with soft output: returns (xhat, iters, marginals) CUDA tensors."""
        import torch

        B, n = priors.shape
        xhat = torch.empty((B, n), dtype=torch.uint8, device=priors.device)
        iters = torch.empty((B,), dtype=torch.int32, device=priors.device)
        marg = torch.zeros_like(priors)
        st = torch.cuda.current_stream(priors.device).cuda_stream
        _lib.check(_lib.load().ldpc_decode_soft(self.h, priors.data_ptr(), None if y0 is None else y0.data_ptr(), B, int(max_iter),
                                                flags, xhat.data_ptr(), iters.data_ptr(), marg.data_ptr(), st))
        return xhat, iters, marg

    def channel_device(self, channel, param, codeword, seed, stream_id, frame0, B, prior_grid=None):
        """Device channel + LLR kernels only: returns (priors or None, y or None) CUDA tensors for frames [frame0, frame0+B).
        ``prior_grid`` = k: the LLRs are rounded to multiples of 2^-k (exact-in-fp32 mode)."""
        import torch

        n = self.code.n
        dt = torch.float64 if self.precision == "f64" else torch.float32
        pri = None if channel == "bec" else torch.empty((B, n), dtype=dt, device="cuda")
        y = None if channel == "biawgn" else torch.empty((B, n), dtype=torch.uint8, device="cuda")
        st = torch.cuda.current_stream().cuda_stream
        _lib.check(_lib.load().ldpc_channel(_lib.CHANNEL[channel] | _lib.ch_prior_grid(prior_grid), _lib.IO_DTYPE[self.precision], float(param), int(codeword), int(seed),
                                            int(stream_id), int(frame0), int(B), n, None if pri is None else pri.data_ptr(),
                                            None if y is None else y.data_ptr(), st))
        return pri, y

    def simulate(self, channel, param, codeword, seed, stream_id, frame0, B, max_iter, counters, flags=0, hist_bins=0):
        """channel -> LLR -> decode -> count for frames [frame0, frame0+B) entirely on the device; ``counters`` is a CUDA
        int64 tensor of 4 + hist_bins entries that is ACCUMULATED into."""
        import torch

        st = torch.cuda.current_stream(counters.device).cuda_stream
        if int(codeword) == -1:
            return self._simulate_random_words(channel, param, seed, stream_id, frame0, B, max_iter, counters, flags, hist_bins, st)
        _lib.check(_lib.load().ldpc_simulate(self.h, _lib.CHANNEL[channel], float(param), int(codeword), int(seed), int(stream_id),
                                             int(frame0), int(B), int(max_iter), flags, hist_bins, counters.data_ptr(), st))

    def simulate_rounds(self, channel, param, codeword, seed, stream_id, frame0, B, rounds, round_stride, max_iter, counters, flags=0, hist_bins=0):
        """``rounds`` passes of ``simulate`` in one call (``ldpc_simulate_rounds``): round r decodes frames frame0 + r * round_stride + [0, B)
        into row r of ``counters`` (CUDA int64 [rounds, 4 + hist_bins], accumulated into).  The LDS-resident erasure decoder runs them as
        ONE launch; every row equals what ``simulate`` gives for that round."""
        import torch

        assert counters.shape == (rounds, 4 + hist_bins) and counters.is_contiguous()
        st = torch.cuda.current_stream(counters.device).cuda_stream
        if int(codeword) == -1:
            for r in range(rounds):
                self._simulate_random_words(channel, param, seed, stream_id, frame0 + r * round_stride, B, max_iter, counters[r], flags, hist_bins, st)
            return
        _lib.check(_lib.load().ldpc_simulate_rounds(self.h, _lib.CHANNEL[channel], float(param), int(codeword), int(seed), int(stream_id),
                                                    int(frame0), int(B), int(rounds), int(round_stride), int(max_iter), flags, hist_bins,
                                                    counters.data_ptr(), st))

    def rounds_per_launch(self):
        """How many Monte-Carlo rounds are worth sending in one ``simulate_rounds`` call: 32 for the LDS-resident erasure decoder (its frame
        positions are refilled across round boundaries; a 65 536-frame round alone is a 0.23 ms launch that mostly ramps up and drains --
        measured at that round size: 286 M frames/s alone, 445 M with 8, 474 M with 16, 490 M with 32 rounds per launch), 1 for everything
        else (their rounds are milliseconds long)."""
        import os

        if self.alg == "BEC" and self.backend != "stream" and self.fused_info()["waves_per_frame"] > 0:
            return int(os.environ.get("LDPC_SIM_ROUNDS_PER_LAUNCH", "32"))
        return 1

    def _simulate_random_words(self, channel, param, seed, stream_id, frame0, B, max_iter, counters, flags, hist_bins, st):
        """``--codeword -1`` (src/main.py:38): every frame sends a random codeword.  A composition on the device.  Codes with a code book
        (the built-in toy codes): channel kernel (picks the word, adds the noise) -> decode -> count against the sent words.  Every other
        code: systematic encoder on random information bits (``Code.encoder()``) -> channel of the sent words -> decode -> count."""
        import torch

        lib = _lib.load()
        if getattr(self, "_cb_dev", None) is None:
            cb = getattr(self.code, "cb", None)
            if cb is None:
                return simulate_random_codewords(self.code, self.code_handle.device, seed, stream_id, frame0, B, self.words_chunk(channel),
                                                 counters, hist_bins, decode_drawn(self, draw_sent(channel, param, seed, stream_id), max_iter, flags))
            self._cb_dev = torch.from_numpy(np.ascontiguousarray(cb, dtype=np.uint8)).cuda()
        n, K = self.code.n, int(self._cb_dev.shape[0])
        dt = torch.float64 if self.precision == "f64" else torch.float32
        step = 1 << 17
        for b0 in range(0, int(B), step):
            nb = min(step, int(B) - b0)
            pri = None if channel == "bec" else torch.empty((nb, n), dtype=dt, device="cuda")
            y = None if channel == "biawgn" else torch.empty((nb, n), dtype=torch.uint8, device="cuda")
            sent = torch.empty((nb, n), dtype=torch.uint8, device="cuda")
            _lib.check(lib.ldpc_channel_words(_lib.CHANNEL[channel], _lib.IO_DTYPE[self.precision], float(param), self._cb_dev.data_ptr(), K,
                                              int(seed), int(stream_id), int(frame0) + b0, nb, n, None if pri is None else pri.data_ptr(),
                                              None if y is None else y.data_ptr(), sent.data_ptr(), st))
            xhat, iters = self.decode_device(pri, y, max_iter, flags)
            _lib.check(lib.ldpc_count_errors_words(xhat.data_ptr(), sent.data_ptr(), iters.data_ptr(), nb, n, hist_bins, counters.data_ptr(), st))

    WORDS_BYTES = 1 << 30  # what the sent words and the channel output of one chunk of the encoded-word path may occupy together

    def words_chunk(self, channel):
        """Frames per chunk of the random-codeword path: what WORDS_BYTES holds of sent words and channel output."""
        esz = 8 if self.precision == "f64" else 4
        per_frame = self.code.n * (1 + (0 if channel == "bec" else esz) + (0 if channel == "biawgn" else 1))
        return max(64, self.WORDS_BYTES // per_frame)

    def channel_sent_device(self, channel, param, sent, seed, stream_id, frame0):
        """``channel_sent`` in this decoder's precision.  -> (priors or None, y or None)."""
        return channel_sent(channel, self.precision, param, sent, seed, stream_id, frame0)

    def fused_info(self):
        out = (ctypes.c_double * 8)()
        _lib.check(_lib.load().ldpc_decoder_fused_info(self.h, out))
        keys = ("waves_per_frame", "lds_gather_cycles_min", "conflict_cycles_identity", "conflict_cycles_planned", "waves_per_cu",
                "lds_bytes_per_frame", "check_rounds", "variable_rounds")
        return dict(zip(keys, list(out)))

    def kernel_name(self, simulate=False):
        """Name of the LDS-resident kernel (as rocprofv3 prints it) this decoder launches; '' on the streaming kernels."""
        buf = ctypes.create_string_buffer(160)
        _lib.check(_lib.load().ldpc_decoder_kernel_name(self.h, 1 if simulate else 0, buf, 160))
        return buf.value.decode()

    def set_profiling(self, on):
        _lib.check(_lib.load().ldpc_decoder_profile(self.h, 1 if on else 0))

    def read_profile(self, reset=True):
        """-> {kernel class: (milliseconds, launches)} accumulated since the last reset (HIP events on the decode stream)."""
        ms = (ctypes.c_double * 4)()
        ln = (ctypes.c_int64 * 4)()
        _lib.check(_lib.load().ldpc_decoder_profile_read(self.h, ms, ln, 1 if reset else 0))
        return {k: (ms[i], ln[i]) for i, k in enumerate(("stream_check_pass", "stream_variable_pass", "fused_decode", "stream_decode_total"))}

    def last_stats(self):
        b, s = ctypes.c_int(0), ctypes.c_int(0)
        _lib.check(_lib.load().ldpc_decoder_last_stats(self.h, ctypes.byref(b), ctypes.byref(s)))
        return _lib.BACKEND_NAME.get(b.value, "?"), s.value

    def grid_violations(self, reset=True):
        """Exact-in-fp32 mode: (count, global frame indices) of the frames set aside by the exactness guard since the last reset."""
        c = ctypes.c_int64(0)
        frames = np.zeros(4095, dtype=np.int64)
        _lib.check(_lib.load().ldpc_decoder_grid_violations(self.h, ctypes.byref(c), frames.ctypes.data, len(frames), 1 if reset else 0))
        return c.value, frames[:min(c.value, len(frames))].copy()

    def _fp64_sibling(self):
        """The same decoder in the reference's own arithmetic: re-decodes the few frames the exactness guard sets aside."""
        if getattr(self, "_sib64", None) is None:
            self._sib64 = DecoderHandle(self.code, self.alg, "f64", "auto", self.code_handle.device)
        return self._sib64

    def decode_device_exact_fp32(self, priors, max_iter, k):
        """fp32 min-sum on priors that lie on the 2^-k grid (``channel_device(..., prior_grid=k)``), guaranteed to return what the fp64
        reference returns for the same priors: frames whose messages left the range where fp32 sums are exact -- the kernel marks them
        -- are decoded again in fp64.  -> (xhat, iters, frames_redone)"""
        xh, it = self.decode_device(priors, None, max_iter, flags=_lib.flag_prior_grid(k))
        self.grid_violations()
        bad = (it < 0).nonzero().flatten()
        if len(bad):
            x64, i64 = self._fp64_sibling().decode_device(priors[bad].double().contiguous(), None, max_iter)
            xh[bad], it[bad] = x64, i64
        return xh, it, int(len(bad))

    def simulate_exact_fp32(self, param, codeword, seed, stream_id, frame0, B, max_iter, counters, k, hist_bins=0):
        """``simulate`` over BI-AWGN in the exact-in-fp32 mode: the LDS-resident fp32 kernel draws priors on the 2^-k grid and counts every
        frame its guard vouches for; the others (listed by the kernel) are generated again, decoded in fp64 and added to ``counters``
        here.  The counters are then those of the fp64 reference on those priors, frame for frame.  -> frames redone in fp64"""
        import torch

        self.simulate("biawgn", param, codeword, seed, stream_id, frame0, B, max_iter, counters, flags=_lib.flag_prior_grid(k), hist_bins=hist_bins)
        cnt, frames = self.grid_violations()
        if cnt > len(frames):
            raise _lib.LdpcHipError("prior grid 2^-%d: %d frames beyond the exactness guard in one call -- the grid is too fine for this operating point" % (k, cnt))
        if cnt:
            h64 = self._fp64_sibling()
            pri = torch.cat([self.channel_device("biawgn", param, codeword, seed, stream_id, int(f), 1, prior_grid=k)[0] for f in frames])
            xh, it = h64.decode_device(pri.double().contiguous(), None, max_iter)
            st = torch.cuda.current_stream().cuda_stream
            _lib.check(_lib.load().ldpc_count_errors(xh.data_ptr(), None, int(codeword), it.data_ptr(), len(frames), self.code.n, hist_bins,
                                                     counters.data_ptr(), st))
        return int(cnt)

    # ---- exact-in-fp32 rounds without a host round trip (montecarlo.DeviceSimulator sends them in blocks)
    REDO_ROWS = 512  # frames of one BLOCK of rounds the fp64 sibling re-decodes at most (a 65 536-frame round at 1-2 dB sets aside 1-15)

    def grid_list_dev(self):
        """Device address of this decoder's redo list ([0] = count, [1..] = global frame indices) -- ``ldpc_decoder_grid_list``."""
        import torch

        p, cap = ctypes.c_void_p(), ctypes.c_int64(0)
        _lib.check(_lib.load().ldpc_decoder_grid_list(self.h, ctypes.byref(p), ctypes.byref(cap), torch.cuda.current_stream().cuda_stream))
        return p.value

    def redo_on_stream(self, param, codeword, seed, stream_id, max_iter, k, counters, redone2, frame_base, round_stride, hist_bins=0):
        """Enqueue, on the CURRENT torch stream, the fp64 re-decode of every frame the guarded kernels set aside since the list was last reset
        (``simulate(..., flags=grid)``, one or several rounds): their priors are drawn again from the device-resident list
        (``ldpc_channel_list``), decoded by the fp64 sibling, counted into the row of their round -- ``counters`` is [rounds, >= 4 + hist_bins],
        round = (frame - frame_base) / round_stride -- and the list is reset.  ``redone2`` (int64[2], device) += [frames counted, 1 if the list
        was longer than REDO_ROWS].  No host synchronisation when the sibling runs on the LDS-resident kernels."""
        import torch

        lib, n, rows = _lib.load(), self.code.n, self.REDO_ROWS
        st = torch.cuda.current_stream().cuda_stream
        lst = self.grid_list_dev()
        if getattr(self, "_redo_pri", None) is None:
            self._redo_pri = torch.zeros((rows, n), dtype=torch.float32, device="cuda")
            self._redo_x = torch.zeros((rows, n), dtype=torch.uint8, device="cuda")
            self._redo_it = torch.zeros((rows,), dtype=torch.int32, device="cuda")
        h64 = self._fp64_sibling()
        _lib.check(lib.ldpc_channel_list(_lib.CHANNEL["biawgn"] | _lib.ch_prior_grid(k), _lib.DTYPE["f32"], float(param), int(codeword), int(seed),
                                         int(stream_id), lst, rows, n, self._redo_pri.data_ptr(), st))
        h64.decode_device(self._redo_pri.double(), None, max_iter, xhat=self._redo_x, iters=self._redo_it)
        nrounds, stride = (counters.shape[0], counters.stride(0)) if counters.dim() == 2 else (1, counters.shape[0])
        _lib.check(lib.ldpc_count_errors_list(self._redo_x.data_ptr(), int(codeword), self._redo_it.data_ptr(), lst, rows, n, hist_bins,
                                              counters.data_ptr(), int(stride), int(frame_base), int(round_stride), int(nrounds),
                                              redone2.data_ptr(), st))
        _lib.check(lib.ldpc_decoder_grid_list_reset(self.h, st))

    def last_repacks(self):
        """Streaming backend: how often the last decode re-formed its tiles from the live frames."""
        r = ctypes.c_int(0)
        _lib.check(_lib.load().ldpc_decoder_last_repacks(self.h, ctypes.byref(r)))
        return r.value

    def chunk_state(self):
        """Streaming backend: (frames per pass, how often a failed reservation halved it)."""
        c, r = ctypes.c_int64(0), ctypes.c_int(0)
        _lib.check(_lib.load().ldpc_decoder_chunk_state(self.h, ctypes.byref(c), ctypes.byref(r)))
        return c.value, r.value


class MlHandle(FamilyHandle):
    """Codebook of a short code resident in HBM + the exhaustive-search kernels (``ldpc_ml_*``)."""
    family = "ldpc_ml"

    def __init__(self, codebook, channel, precision="f64", device=None):
        self.cb = np.ascontiguousarray(codebook, dtype=np.uint8)
        self.K, self.n = self.cb.shape
        self.W = (self.K + 31) // 32
        self.channel, self.precision = channel, precision
        self.device = current_device() if device is None else device
        self._create(self.device, self.cb.ctypes.data, self.K, self.n)

    def obs_dtype(self):
        import torch

        if self.channel != "biawgn":
            return torch.uint8
        return torch.float64 if self.precision == "f64" else torch.float32

    def decode_device(self, y, coef, pick=None, want_mask=True):
        """y: contiguous CUDA tensor [B,n] (observations / symbols) -> dict of CUDA tensors: index, ties, best, xhat[, tie_mask]."""
        import torch

        if not y.is_cuda or not y.is_contiguous() or y.dtype != self.obs_dtype() or y.shape[1] != self.n:
            raise ValueError("y must be a contiguous CUDA tensor [B,%d] of dtype %s" % (self.n, self.obs_dtype()))
        B = y.shape[0]
        out = dict(index=torch.empty(B, dtype=torch.int32, device=y.device), ties=torch.empty(B, dtype=torch.int32, device=y.device),
                   best=torch.empty(B, dtype=torch.float64, device=y.device),
                   xhat=torch.empty((B, self.n), dtype=torch.uint8, device=y.device))
        if want_mask:
            out["tie_mask"] = torch.empty((B, self.W), dtype=torch.int32, device=y.device)
        if B == 0:
            return out
        c2 = (ctypes.c_double * 2)(float(coef[0]), float(coef[1]))
        st = torch.cuda.current_stream(y.device).cuda_stream
        _lib.check(_lib.load().ldpc_ml_decode(self.h, _lib.CHANNEL[self.channel], _lib.DTYPE[self.precision], c2, y.data_ptr(), B,
                                              None if pick is None else pick.data_ptr(), out["index"].data_ptr(),
                                              out["ties"].data_ptr(), out["tie_mask"].data_ptr() if want_mask else None,
                                              out["best"].data_ptr(), out["xhat"].data_ptr(), st))
        return out

    def simulate(self, channel, param, codeword, seed, stream_id, frame0, B, max_iter, counters, flags=0, hist_bins=0):
        """Same call shape as DecoderHandle.simulate (max_iter / flags / hist_bins have no meaning here)."""
        import torch

        st = torch.cuda.current_stream(counters.device).cuda_stream
        _lib.check(_lib.load().ldpc_ml_simulate(self.h, _lib.CHANNEL[channel], _lib.DTYPE[self.precision], float(param), int(codeword),
                                                int(seed), int(stream_id), int(frame0), int(B), counters.data_ptr(), st))


class BecMlHandle(FamilyHandle):
    """ML decoding over the BEC for a code without a code book (``ldpc_bec_ml_*``): peeling, then GF(2) elimination of the residual
    system on the device, one wave per frame that keeps erasures."""
    family = "ldpc_bec_ml"

    def __init__(self, code, device=None):
        self._create_on_code(code, device)

    def words_chunk(self, channel):
        return 1 << 17

    def decode_device(self, y, seed, stream_id=0, frame0=0):
        """y: contiguous CUDA uint8 tensor [B, n] of symbols {0, 1, 2} -> (xhat uint8 [B, n], nullity int32 [B]) for frames
        [frame0, frame0 + B) (the tie-break draws are keyed by (seed, stream_id, global frame index))."""
        import torch

        n = self.code.n
        if not y.is_cuda or y.dtype != torch.uint8 or not y.is_contiguous() or y.dim() != 2 or y.shape[1] != n:
            raise ValueError("y must be a contiguous CUDA uint8 tensor [B, %d]" % n)
        B = y.shape[0]
        xhat = torch.empty((B, n), dtype=torch.uint8, device=y.device)
        nul = torch.empty((B,), dtype=torch.int32, device=y.device)
        if B:
            st = torch.cuda.current_stream(y.device).cuda_stream
            _lib.check(_lib.load().ldpc_bec_ml_decode(self.h, y.data_ptr(), B, int(seed), int(stream_id), int(frame0), xhat.data_ptr(),
                                                      nul.data_ptr(), st))
        return xhat, nul

    def solve_bits(self, bits, erased, seed, stream_id=0, frame0=0):
        """``ldpc_bec_ml_solve`` on peeled packed frames (``DecoderHandle.decode_device_bits`` of an erasure decoder, max_iter <= 0):
        bits / erased int32 CUDA [B, ceil(n/32)] -> (resolved words int32 [B, W], nullity int32 [B])."""
        import torch

        B = bits.shape[0]
        out = torch.empty_like(bits)
        nul = torch.empty((B,), dtype=torch.int32, device=bits.device)
        if B:
            st = torch.cuda.current_stream(bits.device).cuda_stream
            _lib.check(_lib.load().ldpc_bec_ml_solve(self.h, bits.data_ptr(), erased.data_ptr(), B, int(seed), int(stream_id), int(frame0),
                                                     out.data_ptr(), nul.data_ptr(), st))
        return out, nul

    def simulate(self, channel, param, codeword, seed, stream_id, frame0, B, max_iter, counters, flags=0, hist_bins=0):
        """Same call shape as DecoderHandle.simulate (max_iter / flags / hist_bins have no meaning here; ITER_SUM stays 0).
        ``codeword == -1``: random codewords from the systematic encoder (``Code.encoder()``) through ``ldpc_channel_sent``."""
        import torch

        if channel != "bec":
            raise ValueError("the elimination ML decoder works on the erasure channel only")
        if B <= 0:
            return
        lib = _lib.load()
        st = torch.cuda.current_stream(counters.device).cuda_stream
        if int(codeword) != -1:
            _lib.check(lib.ldpc_bec_ml_simulate(self.h, float(param), int(codeword), int(seed), int(stream_id), int(frame0), int(B),
                                                counters.data_ptr(), st))
            return

        def decode(sent, first):
            y = channel_sent("bec", "f32", param, sent, seed, stream_id, first)[1]
            return self.decode_device(y, seed, stream_id, first)[0], None

        simulate_random_codewords(self.code, self.device, seed, stream_id, frame0, B, self.words_chunk(channel), counters, 0, decode)


class OsdHandle(FamilyHandle):
    """Ordered-statistics post-processing of an LLR decoder (``ldpc_osd_*``): the frames BP leaves without a codeword are decoded again
    from its soft output, one wave per frame.  ``bp`` is the ``DecoderHandle`` (fp32 / fp64 MSA, SPA, NMSA or QMSA, same code) that runs in
    front; ``order`` in {0, 1} and ``depth`` >= 0 are read at every call."""
    family = "ldpc_osd"

    def __init__(self, bp, order=0, depth=64):
        self.bp, self.code, self.code_handle = bp, bp.code, bp.code_handle
        self.device, self.precision = bp.code_handle.device, bp.precision
        self.order, self.depth = int(order), int(depth)
        self._create(self.code_handle.h)

    def words_chunk(self, channel):
        return 1 << 17

    def solve(self, post, prior, order=None, depth=None, want_cost=True):
        """``ldpc_osd_solve``: post / prior contiguous CUDA tensors [B, n] of one dtype (float32 or float64) -> (words int32 [B, ceil(n/32)]
        in the layout of ``decode_device_bits``, pick int32 [B], cost float64 [B] or None)."""
        import torch

        n = self.code.n
        for t in (post, prior):
            if not t.is_cuda or not t.is_contiguous() or t.dim() != 2 or t.shape[1] != n or t.dtype not in (torch.float32, torch.float64):
                raise ValueError("post and prior must be contiguous CUDA float32 / float64 tensors [B, %d]" % n)
        if post.dtype != prior.dtype or post.shape != prior.shape:
            raise ValueError("post and prior must have one dtype and one shape")
        B = post.shape[0]
        bits = torch.empty((B, (n + 31) // 32), dtype=torch.int32, device=post.device)
        pick = torch.empty((B,), dtype=torch.int32, device=post.device)
        cost = torch.empty((B,), dtype=torch.float64, device=post.device) if want_cost else None
        if B:
            st = torch.cuda.current_stream(post.device).cuda_stream
            _lib.check(_lib.load().ldpc_osd_solve(self.h, _lib.DTYPE["f64" if post.dtype == torch.float64 else "f32"], post.data_ptr(),
                                                  prior.data_ptr(), B, int(self.order if order is None else order),
                                                  int(self.depth if depth is None else depth), bits.data_ptr(), pick.data_ptr(),
                                                  None if cost is None else cost.data_ptr(), st))
        return bits, pick, cost

    def decode_device(self, priors, y0, max_iter, flags=0, order=None, depth=None, bp=None):
        """``ldpc_osd_decode``: BP by ``bp`` (default: the handle's own decoder), then OSD -> (xhat uint8 [B, n], BP's iters int32 [B],
        pick int32 [B]: -1 where BP's word was a codeword and is returned as it is)."""
        import torch

        n, B = self.code.n, priors.shape[0]
        bp = self.bp if bp is None else bp
        xhat = torch.empty((B, n), dtype=torch.uint8, device=priors.device)
        iters = torch.empty((B,), dtype=torch.int32, device=priors.device)
        pick = torch.empty((B,), dtype=torch.int32, device=priors.device)
        if not priors.is_cuda or not priors.is_contiguous() or priors.dim() != 2 or priors.shape[1] != n:
            raise ValueError("priors must be a contiguous CUDA tensor [B, %d]" % n)
        if y0 is not None and (y0.dtype != torch.uint8 or not y0.is_contiguous() or not y0.is_cuda):
            raise ValueError("y0 must be a contiguous CUDA uint8 tensor")
        if B:
            st = torch.cuda.current_stream(priors.device).cuda_stream
            _lib.check(_lib.load().ldpc_osd_decode(self.h, bp.h, priors.data_ptr(), None if y0 is None else y0.data_ptr(), B, int(max_iter), flags,
                                                   int(self.order if order is None else order), int(self.depth if depth is None else depth),
                                                   xhat.data_ptr(), iters.data_ptr(), pick.data_ptr(), st))
        return xhat, iters, pick

    def simulate(self, channel, param, codeword, seed, stream_id, frame0, B, max_iter, counters, flags=0, hist_bins=0):
        """Same call shape as DecoderHandle.simulate: channel -> LLR -> BP -> OSD -> count on the device; ITER_SUM and the histogram are
        BP's.  ``codeword == -1``: random codewords from the systematic encoder (``Code.encoder()``) through ``ldpc_channel_sent``."""
        import torch

        if channel not in ("biawgn", "bsc"):
            raise ValueError("ordered-statistics post-processing works on the LLR channels (biawgn, bsc); the bec has ML")
        if B <= 0:
            return
        lib = _lib.load()
        st = torch.cuda.current_stream(counters.device).cuda_stream
        if int(codeword) != -1:
            _lib.check(lib.ldpc_osd_simulate(self.h, self.bp.h, _lib.CHANNEL[channel], float(param), int(codeword), int(seed), int(stream_id),
                                             int(frame0), int(B), int(max_iter), flags, self.order, self.depth, hist_bins, counters.data_ptr(), st))
            return

        simulate_random_codewords(self.code, self.device, seed, stream_id, frame0, B, self.words_chunk(channel), counters, hist_bins,
                                  decode_drawn(self, draw_sent(channel, param, seed, stream_id), max_iter, flags))


class HardHandle(FamilyHandle):
    """Bit-sliced Gallager-B hard-decision decoder (``ldpc_hard_*``): one bit per message, 32 frames per machine word.  ``backend``:
    "stream" (planes in HBM, any code), "fused" (one slab per workgroup in the LDS; refused for a code that does not fit) or "auto"."""
    family = "ldpc_hard"

    def __init__(self, code, backend="auto", device=None, threshold=0):
        self.backend = backend
        self._create_on_code(code, device, _lib.BACKEND[backend])
        if threshold:
            self.set_threshold(threshold)

    def set_threshold(self, t):
        _lib.check(_lib.load().ldpc_hard_set_threshold(self.h, int(t)))

    def threshold(self):
        t = ctypes.c_int(0)
        _lib.check(_lib.load().ldpc_hard_get_threshold(self.h, ctypes.byref(t)))
        return t.value

    def last_backend(self):
        """Kernels of the last decode / simulate: "stream" or "fused" (before the first call: what the handle will use)."""
        b = ctypes.c_int(0)
        _lib.check(_lib.load().ldpc_hard_last_backend(self.h, ctypes.byref(b)))
        return _lib.BACKEND_NAME.get(b.value, "?")

    def info(self):
        out = (ctypes.c_double * 4)()
        _lib.check(_lib.load().ldpc_hard_info(self.h, out))
        return dict(zip(("lds_bytes_per_slab", "frames_per_slab", "slabs_per_cu", "workgroups"), (int(v) for v in out)))

    def _check_y(self, y):
        import torch

        if not hasattr(y, "is_cuda") or not y.is_cuda or y.dtype != torch.uint8 or not y.is_contiguous() or y.dim() != 2 or y.shape[1] != self.code.n:
            raise ValueError("y must be a contiguous CUDA uint8 tensor [B, %d]" % self.code.n)

    def decode_device(self, y, max_iter, flags=0):
        """y: contiguous CUDA uint8 [B, n] in {0, 1} -> (xhat uint8 [B, n], iters int32 [B])."""
        import torch

        self._check_y(y)
        B, n = y.shape
        xhat = torch.empty((B, n), dtype=torch.uint8, device=y.device)
        iters = torch.empty((B,), dtype=torch.int32, device=y.device)
        if B:
            st = torch.cuda.current_stream(y.device).cuda_stream
            _lib.check(_lib.load().ldpc_hard_decode(self.h, y.data_ptr(), B, int(max_iter), flags, xhat.data_ptr(), None, iters.data_ptr(), st))
        return xhat, iters

    def decode_device_bits(self, y, max_iter, flags=0):
        """Packed decisions -> (xhat_bits int32 [B, ceil(n/32)] in the layout of ``DecoderHandle.decode_device_bits``, iters)."""
        import torch

        self._check_y(y)
        B, W = y.shape[0], (self.code.n + 31) // 32
        bits = torch.empty((B, W), dtype=torch.int32, device=y.device)
        iters = torch.empty((B,), dtype=torch.int32, device=y.device)
        if B:
            st = torch.cuda.current_stream(y.device).cuda_stream
            _lib.check(_lib.load().ldpc_hard_decode(self.h, y.data_ptr(), B, int(max_iter), flags, None, bits.data_ptr(), iters.data_ptr(), st))
        return bits, iters

    def simulate(self, channel, param, codeword, seed, stream_id, frame0, B, max_iter, counters, flags=0, hist_bins=0):
        """Same call shape as DecoderHandle.simulate: channel -> hard decisions -> decode -> count on the device (``ldpc_hard_simulate``).
        ``codeword == -1``: random codewords from the systematic encoder (``Code.encoder()``) through ``ldpc_channel_sent``."""
        import torch

        if channel not in ("biawgn", "bsc"):
            raise ValueError("a hard-decision decoder works on the bsc and on the sliced biawgn; it has no erasures to work on")
        if B <= 0:
            return
        lib = _lib.load()
        st = torch.cuda.current_stream(counters.device).cuda_stream
        if int(codeword) != -1:
            _lib.check(lib.ldpc_hard_simulate(self.h, _lib.CHANNEL[channel], float(param), int(codeword), int(seed), int(stream_id), int(frame0),
                                              int(B), int(max_iter), flags, hist_bins, counters.data_ptr(), st))
            return

        def decode(sent, first):
            pri, y = channel_sent(channel, "f32", param, sent, seed, stream_id, first, priors=channel == "biawgn")
            if y is None:
                y = (pri < 0).to(torch.uint8)  # the word sliced at prior < 0
            return self.decode_device(y, max_iter, flags)

        simulate_random_codewords(self.code, self.device, seed, stream_id, frame0, B, self.words_chunk(channel), counters, hist_bins, decode)

    def words_chunk(self, channel):
        return max(2048, min(1 << 17, (1 << 28) // self.code.n))


class LqmsaHandle(FixedPointLayers, FamilyHandle):
    """Layered fixed-point min-sum with the frame resident in the LDS as integers (``ldpc_lqmsa_*``): one workgroup per frame, int16
    marginals, int8 check messages; priors in fp32 or fp64, quantised on load."""
    family = "ldpc_lqmsa"  # the handle family of the C ABI the calls below go to (QcHandle: the same call shapes under ldpc_qc_*)
    precision = "f32"  # the type ``simulate`` draws its priors in (``decode_device`` takes fp32 and fp64; the integers are the same)

    def __init__(self, code, device=None, bits=6, frac_bits=2, scale=0.8125, offset=0):
        self._create_on_code(code, device)
        self.set_fixed_point(bits, frac_bits, scale, offset)

    def info(self):
        out = (ctypes.c_double * 4)()
        _lib.check(self._fn("info")(self.h, out))
        return dict(zip(("lds_bytes_per_frame", "waves_per_frame", "frames_per_cu", "workgroups"), (int(v) for v in out)))

    def decode_device(self, priors, y0, max_iter, flags=0, bits=False, soft=False):
        """priors: contiguous CUDA float32 / float64 [B, n]; y0: CUDA uint8 [B, n] or None -> (xhat uint8 [B, n], iters int32 [B]), with
        ``bits`` the packed words int32 [B, ceil(n/32)] and with ``soft`` the marginals in levels int16 [B, n] appended."""
        import torch

        n = self.code.n
        if not getattr(priors, "is_cuda", False) or priors.dtype not in (torch.float32, torch.float64) or not priors.is_contiguous() \
                or priors.dim() != 2 or priors.shape[1] != n:
            raise ValueError("priors must be a contiguous CUDA float32 or float64 tensor [B, %d]" % n)
        B = priors.shape[0]
        if y0 is not None and (not getattr(y0, "is_cuda", False) or y0.dtype != torch.uint8 or not y0.is_contiguous() or tuple(y0.shape) != (B, n)):
            raise ValueError("y0 must be a contiguous CUDA uint8 tensor [%d, %d]" % (B, n))
        dev = priors.device
        xhat = torch.empty((B, n), dtype=torch.uint8, device=dev)
        iters = torch.empty((B,), dtype=torch.int32, device=dev)
        words = torch.empty((B, (n + 31) // 32), dtype=torch.int32, device=dev) if bits else None
        marg = torch.empty((B, n), dtype=torch.int16, device=dev) if soft else None
        if B:
            st = torch.cuda.current_stream(dev).cuda_stream
            _lib.check(self._fn("decode")(self.h, _lib.DTYPE["f64" if priors.dtype == torch.float64 else "f32"], priors.data_ptr(),
                                          None if y0 is None else y0.data_ptr(), B, int(max_iter), flags, xhat.data_ptr(),
                                          None if words is None else words.data_ptr(), iters.data_ptr(),
                                          None if marg is None else marg.data_ptr(), st))
        return (xhat, iters) + ((words,) if bits else ()) + ((marg,) if soft else ())

    def simulate(self, channel, param, codeword, seed, stream_id, frame0, B, max_iter, counters, flags=0, hist_bins=0):
        """Same call shape as DecoderHandle.simulate: channel -> LLR -> decode -> count on the device (``ldpc_lqmsa_simulate``).
        ``codeword == -1``: random codewords from the systematic encoder (``Code.encoder()``) through ``ldpc_channel_sent``."""
        import torch

        if channel not in ("biawgn", "bsc"):
            raise ValueError("layered fixed-point min-sum works on the LLR channels (biawgn, bsc)")
        if B <= 0:
            return
        lib = _lib.load()
        st = torch.cuda.current_stream(counters.device).cuda_stream
        if int(codeword) != -1:
            _lib.check(self._fn("simulate")(self.h, _lib.CHANNEL[channel], float(param), int(codeword), int(seed), int(stream_id), int(frame0),
                                            int(B), int(max_iter), flags, hist_bins, counters.data_ptr(), st))
            return

        simulate_random_codewords(self.code, self.device, seed, stream_id, frame0, B, self.words_chunk(channel), counters, hist_bins,
                                  decode_drawn(self, draw_sent(channel, param, seed, stream_id), max_iter, flags))

    def words_chunk(self, channel):
        return max(2048, min(1 << 17, (1 << 26) // self.code.n))


class QcHandle(LqmsaHandle):
    """Layered fixed-point min-sum on a quasi-cyclic code, shift-addressed (``ldpc_qc_*``): LqmsaHandle's call shapes and outputs with every
    block row of the base matrix one layer; the library finds the shifts for the lifting size ``Z`` from the code's edge list."""
    family = "ldpc_qc"

    def __init__(self, code, Z, device=None, bits=6, frac_bits=2, scale=0.8125, offset=0, pack=1):
        self._create_on_code(code, device, int(Z))
        self.set_fixed_point(bits, frac_bits, scale, offset)
        if pack != 1:
            self.set_pack(pack)

    def set_pack(self, P):
        """Frames per wave (``ldpc_qcpack_set``): 0 the rule's pick (``qc.qc_pack``), 1 one frame per workgroup, P >= 2 needs Z <= 32,
        P Z <= 64 and P strides of LDS.  No result depends on it."""
        _lib.check(_lib.load().ldpc_qcpack_set(self.h, int(P)))

    def pack(self):
        """-> (frames per wave in force, the rule's pick)"""
        P, pick = ctypes.c_int32(0), ctypes.c_int32(0)
        _lib.check(_lib.load().ldpc_qcpack_get(self.h, ctypes.byref(P), ctypes.byref(pick)))
        return P.value, pick.value

    def set_layers(self, layers=None):
        raise TypeError("the layers of a quasi-cyclic decoder are its block rows: set_order")

    layers = set_layers

    def base(self):
        """-> (base matrix int32 [mb, nb] with -1 for a zero block, Z) as the library detected it (``ldpc_qc_get_base``)"""
        mb, nb, Z = ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int32(0)
        _lib.check(self._fn("get_base")(self.h, ctypes.byref(mb), ctypes.byref(nb), ctypes.byref(Z), None))
        shifts = np.empty((mb.value, nb.value), dtype=np.int32)
        _lib.check(self._fn("get_base")(self.h, ctypes.byref(mb), ctypes.byref(nb), ctypes.byref(Z), shifts.ctypes.data))
        return shifts, Z.value

    def set_order(self, order=None):
        """``order``: the block row processed at each position, a permutation of 0 .. mb - 1; None: the natural order."""
        if order is None:
            _lib.check(self._fn("set_order")(self.h, None, 0))
            return
        o = np.ascontiguousarray(order, dtype=np.int32)
        _lib.check(self._fn("set_order")(self.h, o.ctypes.data, o.size))

    def order(self):
        mb = ctypes.c_int32(0)
        _lib.check(self._fn("get_order")(self.h, ctypes.byref(mb), None))
        o = np.empty(mb.value, dtype=np.int32)
        _lib.check(self._fn("get_order")(self.h, ctypes.byref(mb), o.ctypes.data))
        return o


class SlqHandle(LqmsaHandle):
    """Layered fixed-point min-sum on the streaming kernels (``ldpc_slq_*``): LqmsaHandle's call shapes and outputs with the integer state
    in HBM tiles (int16 marginals, int8 messages, lane = frame), for any code -- no LDS rule."""
    family = "ldpc_slq"

    def info(self):
        out = (ctypes.c_double * 4)()
        _lib.check(self._fn("info")(self.h, out))
        return dict(zip(("state_bytes_per_frame", "tiles_per_chunk", "layers", "launches_per_sweep"), (int(v) for v in out)))

    def profile(self, on=True):
        """Per-kernel timing with HIP events on the decode stream; a decode then ends with a stream synchronise."""
        _lib.check(self._fn("profile")(self.h, 1 if on else 0, None, None, 0))

    def read_profile(self, reset=True):
        """-> {kernel class: (milliseconds, launches)} accumulated since the last reset."""
        ms, ln = (ctypes.c_double * 3)(), (ctypes.c_int64 * 3)()
        _lib.check(self._fn("profile")(self.h, -1, ms, ln, 1 if reset else 0))
        return {k: (ms[i], ln[i]) for i, k in enumerate(("layer_passes", "decision_pass", "decode_total"))}

    def last_stats(self):
        """-> (sweeps enqueued by the last decode, frame repacks, chunks)"""
        out = (ctypes.c_int32 * 3)()
        _lib.check(self._fn("last_stats")(self.h, out))
        return tuple(out)


class AdmmHandle(FamilyHandle):
    """ADMM LP decoder workspace on one GPU (``ldpc_admm_*``)."""
    family = "ldpc_admm"

    def __init__(self, code, device=None):
        self._create_on_code(code, device)

    def decode_device(self, gamma, mu, eps, max_iter):
        """gamma: contiguous CUDA float64 [B,n] -> (x float64 [B,n] before pseudo_to_cw, iters int32 [B], converged uint8 [B])."""
        import torch

        if not gamma.is_cuda or gamma.dtype != torch.float64 or not gamma.is_contiguous() or gamma.shape[1] != self.code.n:
            raise ValueError("gamma must be a contiguous CUDA float64 tensor [B,%d]" % self.code.n)
        B = gamma.shape[0]
        x = torch.empty_like(gamma)
        iters = torch.empty(B, dtype=torch.int32, device=gamma.device)
        conv = torch.empty(B, dtype=torch.uint8, device=gamma.device)
        if B == 0:  # zero-size tensors have no storage to point at
            return x, iters, conv
        st = torch.cuda.current_stream(gamma.device).cuda_stream
        _lib.check(_lib.load().ldpc_admm_decode(self.h, gamma.data_ptr(), B, float(mu), float(eps), int(max_iter), x.data_ptr(),
                                                iters.data_ptr(), conv.data_ptr(), st))
        return x, iters, conv

    # knobs of the simulate() composition below, set by admm.ADMM
    mu, eps, allow_pseudo, on_iters = 3.0, 1e-5, False, None

    def last_repacks(self):
        """How often the last decode re-formed its tiles from the live frames."""
        r = ctypes.c_int(0)
        _lib.check(_lib.load().ldpc_admm_last_repacks(self.h, ctypes.byref(r)))
        return r.value

    def last_backend(self):
        """Kernels of the last decode: "stream" (state in HBM) or "lds" (one workgroup per frame, state in the LDS)."""
        r = ctypes.c_int(0)
        _lib.check(_lib.load().ldpc_admm_last_backend(self.h, ctypes.byref(r)))
        return "lds" if r.value == 1 else "stream"

    def simulate(self, channel, param, codeword, seed, stream_id, frame0, B, max_iter, counters, flags=0, hist_bins=0):
        """Same call shape as DecoderHandle.simulate: device channel kernel -> LLRs -> ADMM -> pseudo_to_cw -> counters, all
        on the GPU (a composition of ldpc_channel / ldpc_admm_decode / torch element-wise ops; no host noise)."""
        import torch

        if B <= 0:
            return
        lib, n = _lib.load(), self.code.n
        st = torch.cuda.current_stream(counters.device).cuda_stream
        step = 1 << 15
        for b0 in range(0, int(B), step):
            nb = min(step, int(B) - b0)
            if channel == "bec":
                y = torch.empty((nb, n), dtype=torch.uint8, device=counters.device)
                _lib.check(lib.ldpc_channel(_lib.CHANNEL[channel], 0, float(param), int(codeword), int(seed), int(stream_id), int(frame0) + b0,
                                            nb, n, None, y.data_ptr(), st))
                gamma = torch.tensor([1e8, -1e8, 0.0], dtype=torch.float64, device=counters.device)[y.long()]  # src/bec.py:41
            else:
                gamma = torch.empty((nb, n), dtype=torch.float64, device=counters.device)
                y = torch.empty((nb, n), dtype=torch.uint8, device=counters.device) if channel == "bsc" else None
                _lib.check(lib.ldpc_channel(_lib.CHANNEL[channel], _lib.DTYPE["f64"], float(param), int(codeword), int(seed), int(stream_id),
                                            int(frame0) + b0, nb, n, gamma.data_ptr(), None if y is None else y.data_ptr(), st))
            x, iters, _ = self.decode_device(gamma.contiguous(), self.mu, self.eps, max_iter)
            if self.allow_pseudo:  # src/math_utils.py:28-34, then `x != x_hat` as src/main.py:41
                x = torch.where(x < 1e-8, torch.zeros_like(x), x)
                x = torch.where(1 - x < 1e-8, torch.ones_like(x), x)
                wrong = x != float(codeword)
            else:
                wrong = (x > .5) != bool(codeword)
            err = wrong.sum(dim=1)
            counters[_lib.CNT_TOT] += nb
            counters[_lib.CNT_WEC] += (err > 0).sum()
            counters[_lib.CNT_BEC] += err.sum()
            counters[_lib.CNT_ITER_SUM] += iters.sum()
            if hist_bins:
                counters[_lib.CNT_HIST0:_lib.CNT_HIST0 + hist_bins] += torch.bincount(iters.clamp(max=hist_bins - 1).long(), minlength=hist_bins)
            if self.on_iters is not None:
                self.on_iters(iters)


def check_pattern_run(channel, exact=False, prior_grid=None):
    """What a transmission pattern cannot be combined with -- ValueError, before any device call."""
    if channel == "bec":
        raise ValueError("a transmission pattern works on the LLR channels (biawgn, bsc): over the bec a punctured bit is simply an erased one")
    if exact:
        raise ValueError("--exact draws its noise on the host for every bit of the mother code and has no transmission pattern")
    if prior_grid is not None:
        raise ValueError("--prior-grid: the exactness guard vouches for the priors the fused kernel draws itself; a transmission pattern draws them outside it")


class PatternHandle:
    """A transmission pattern (``ratematch.Pattern``) around the handle of an LLR decoder: ``simulate`` in the call shape of
    ``DecoderHandle.simulate``, so ``montecarlo.DeviceSimulator`` and the multi-GPU driver take it as they take ``inner``.  Per chunk of
    ``inner.words_chunk(channel)`` frames: the sent words (``codeword == -1``; none for the all-zero / all-one word) ->
    ``ldpc_channel_pattern`` in the inner handle's precision -> the inner handle's decode of given priors (``decode_drawn``) ->
    ``ldpc_count_errors_pattern``.  Every draw is keyed by the global frame index, so sharding and chunking change no counter.

    Served: ``DecoderHandle`` (SPA, MSA, NMSA, QMSA, LMSA), ``OsdHandle``, ``LqmsaHandle``, ``QcHandle``, ``SlqHandle``.  Refused
    (ValueError, before any device call): ``HardHandle``, ``AdmmHandle``, ``MlHandle``, ``BecMlHandle``, the erasure decoder, the bec channel
    and the prior-grid flag."""
    CHUNK = None  # frames per chunk; None: ``inner.words_chunk(channel)`` (a test forces a small one here)
    REFUSED = ((HardHandle, "a hard-decision decoder passes one bit per message and has no erasure to start a punctured bit from"),
               (AdmmHandle, "the ADMM decoder has no transmission pattern: it is the LLR decoders (SPA, MSA and the min-sum variants, OSD) that take one"),
               (MlHandle, "codebook ML has no transmission pattern: it is the LLR decoders (SPA, MSA and the min-sum variants, OSD) that take one"),
               (BecMlHandle, "ML over the erasure channel has no transmission pattern: a punctured bit is simply an erased one there"))

    def __init__(self, inner, pattern, short_llr=32.0):
        for cls, why in self.REFUSED:
            if isinstance(inner, cls):
                raise ValueError(why)
        if not isinstance(inner, (DecoderHandle, OsdHandle, LqmsaHandle)) or getattr(inner, "alg", None) == "BEC":
            raise ValueError("a transmission pattern wraps the handle of an LLR decoder (DecoderHandle but the erasure decoder, OsdHandle, LqmsaHandle, QcHandle, SlqHandle)")
        if pattern.n != inner.code.n:
            raise ValueError("a pattern of %d variables on a code of %d" % (pattern.n, inner.code.n))
        short_llr = float(short_llr)
        if not 0.0 < short_llr < float("inf"):
            raise ValueError("short_llr must be finite and > 0 (got %r)" % short_llr)
        self.inner, self.pattern, self.short_llr = inner, pattern, short_llr
        self.code, self.device, self.precision = inner.code, inner.code_handle.device, inner.precision

    def kind_device(self):
        """The pattern's ``kind`` as a CUDA uint8 tensor [n] on the handle's device, kept on the handle."""
        import torch

        if getattr(self, "_kind_dev", None) is None:
            self._kind_dev = torch.from_numpy(self.pattern.kind).to(torch.device("cuda", self.device))
        return self._kind_dev

    def ones_words(self, B):
        """``B`` all-one words, CUDA uint8 [B, n] (kept, grown on demand): what ``codeword == 1`` hands to ``ldpc_channel_pattern``, which for
        the all-one word without sent words would read the pattern back and wait for the stream at every call -- the check it makes
        there (no shortened bit) is made on the host in ``simulate``."""
        import torch

        if getattr(self, "_ones", None) is None or self._ones.shape[0] < B:
            self._ones = torch.ones((int(B), self.code.n), dtype=torch.uint8, device=torch.device("cuda", self.device))
        return self._ones[:int(B)]

    def sent_words(self, seed, stream_id, frame0, B):
        """Random codewords of the shortened code for frames [frame0, frame0 + B), CUDA uint8 [B, n], zero on the shortened set: the words
        of ``Code.encoder()`` of ``pattern.shortened_code(code)`` scattered through its index map; with no shortened bit exactly the
        words of ``Code.encoder()`` of the code itself."""
        import torch

        if self.pattern.shortened.size == 0:
            return self.code.encoder().handle(self.device).encode_random(seed, stream_id, frame0, B)
        short, index = self.pattern.shortened_code(self.code)
        words = short.encoder().handle(self.device).encode_random(seed, stream_id, frame0, B)
        if getattr(self, "_index_dev", None) is None:
            self._index_dev = torch.from_numpy(index).to(words.device)
        return torch.zeros((int(B), self.code.n), dtype=torch.uint8, device=words.device).index_copy_(1, self._index_dev, words)

    def simulate(self, channel, param, codeword, seed, stream_id, frame0, B, max_iter, counters, flags=0, hist_bins=0):
        """Same call shape as DecoderHandle.simulate; ``counters`` (CUDA int64 [4 + hist_bins]) is accumulated into.  BEC counts the bit errors
        over the sent and the punctured variables (``pattern.n_counted`` per frame)."""
        import torch

        check_pattern_run(channel, prior_grid=_lib.prior_grid_of_flags(flags))
        codeword = int(codeword)
        if codeword not in (-1, 0, 1):
            raise ValueError("codeword is 0, 1 or -1 (a random codeword per frame)")
        if codeword == 1 and self.pattern.shortened.size:
            raise ValueError("the all-one word is no codeword of the shortened code")
        if B <= 0:
            return
        lib, n, kind = _lib.load(), self.code.n, self.kind_device()
        st = torch.cuda.current_stream(counters.device).cuda_stream
        chunk = int(self.CHUNK or self.inner.words_chunk(channel))
        last = int(frame0) + int(B)
        decode = decode_drawn(self.inner, lambda precision, sent, first: channel_pattern(
            channel, precision, param, sent, 0, kind, self.short_llr, seed, stream_id, first, min(chunk, last - first)), max_iter, flags)
        for first in range(int(frame0), last, chunk):
            nb = min(chunk, last - first)
            sent = self.sent_words(seed, stream_id, first, nb) if codeword == -1 else None
            xhat, iters = decode(self.ones_words(nb) if codeword == 1 else sent, first)
            _lib.check(lib.ldpc_count_errors_pattern(xhat.data_ptr(), None if sent is None else sent.data_ptr(), max(codeword, 0), kind.data_ptr(),
                                                     None if iters is None else iters.data_ptr(), nb, n, hist_bins, counters.data_ptr(), st))


def _io_dtype(precision):
    import torch

    return torch.float64 if precision == "f64" else torch.float32


def harq_transmit(channel, precision, param, sent, codeword, kind, cnt, first, short_llr, seed, stream_id, frame0, B=None, src=None, orig=None,
                  soft_old=None):
    """``ldpc_harq_transmit``: one transmission of a HARQ schedule into a new soft buffer.  ``kind`` / ``cnt`` / ``first`` CUDA uint8 [n] (the
    pattern and the transmission's row of ``ratematch.Harq.cnt`` / ``.first``); ``sent`` CUDA uint8 [rows, n] or None for the
    all-``codeword`` word; ``src`` / ``orig`` CUDA int64 [B_out] or None for the identity (the row of ``soft_old`` an output row continues;
    its frame, and its row of ``sent``, relative to ``frame0``); ``soft_old`` in ``precision`` or None for the first transmission.
    ``B`` is needed when neither list is given.  -> the new soft buffer [B_out, n]: what the decoder gets as priors."""
    import torch

    n = kind.shape[0]
    B_out = int(src.shape[0] if src is not None else orig.shape[0] if orig is not None else B)
    dt = _io_dtype(precision)
    for name, idx in (("src", src), ("orig", orig)):
        if idx is not None and (idx.dtype != torch.int64 or not idx.is_contiguous() or not idx.is_cuda or tuple(idx.shape) != (B_out,)):
            raise ValueError("%s must be a contiguous CUDA int64 tensor [%d]" % (name, B_out))
    if soft_old is not None and (soft_old.dtype != dt or not soft_old.is_contiguous() or not soft_old.is_cuda or soft_old.dim() != 2 or soft_old.shape[1] != n):
        raise ValueError("soft_old must be a contiguous CUDA tensor [rows, %d] of dtype %s" % (n, dt))
    if sent is not None and (sent.dtype != torch.uint8 or not sent.is_contiguous() or not sent.is_cuda or sent.dim() != 2 or sent.shape[1] != n):
        raise ValueError("sent must be a contiguous CUDA uint8 tensor [rows, %d]" % n)
    for tab in (cnt, first):
        if tab.dtype != torch.uint8 or not tab.is_contiguous() or not tab.is_cuda or tuple(tab.shape) != (n,):
            raise ValueError("cnt and first must be contiguous CUDA uint8 tensors [%d]" % n)
    soft = torch.empty((B_out, n), dtype=dt, device=kind.device)
    st = torch.cuda.current_stream(kind.device).cuda_stream
    _lib.check(_lib.load().ldpc_harq_transmit(
        _lib.CHANNEL[channel], _lib.IO_DTYPE[precision], float(param), None if sent is None else sent.data_ptr(), 0 if sent is None else sent.shape[0],
        int(codeword), kind.data_ptr(), cnt.data_ptr(), first.data_ptr(), float(short_llr), int(seed), int(stream_id), int(frame0),
        None if src is None else src.data_ptr(), None if orig is None else orig.data_ptr(), None if soft_old is None else soft_old.data_ptr(),
        0 if soft_old is None else soft_old.shape[0], B_out, n, soft.data_ptr(), st))
    return soft


def harq_syndrome(code_h, xhat):
    """``ldpc_harq_syndrome``: -> fail CUDA uint8 [B], 1 where ``xhat`` (CUDA uint8 [B, n]) leaves a check of ``code_h`` (a ``CodeHandle``)
    unsatisfied."""
    import torch

    if xhat.dtype != torch.uint8 or not xhat.is_contiguous() or not xhat.is_cuda or xhat.dim() != 2 or xhat.shape[1] != code_h.code.n:
        raise ValueError("xhat must be a contiguous CUDA uint8 tensor [B, %d]" % code_h.code.n)
    fail = torch.empty((xhat.shape[0],), dtype=torch.uint8, device=xhat.device)
    _lib.check(_lib.load().ldpc_harq_syndrome(code_h.h, xhat.data_ptr(), xhat.shape[0], fail.data_ptr(), torch.cuda.current_stream(xhat.device).cuda_stream))
    return fail


def harq_tally(xhat, sent, codeword, kind, iters, fail, orig, hist_bins, t, T, tx_bits, counters):
    """``ldpc_harq_tally``: transmission ``t`` of ``T`` accumulated into ``counters`` (CUDA int64 [4 + hist_bins + T + 2])."""
    import torch

    B, n = xhat.shape
    if counters.dtype != torch.int64 or not counters.is_contiguous() or counters.numel() != 4 + int(hist_bins) + int(T) + 2:
        raise ValueError("counters must be a contiguous CUDA int64 tensor [%d]" % (4 + int(hist_bins) + int(T) + 2))
    if tuple(fail.shape) != (B,) or fail.dtype != torch.uint8 or (orig is not None and (tuple(orig.shape) != (B,) or orig.dtype != torch.int64)) \
            or (iters is not None and (tuple(iters.shape) != (B,) or iters.dtype != torch.int32)) or tuple(kind.shape) != (n,) \
            or (sent is not None and (sent.dim() != 2 or sent.shape[1] != n or not sent.is_contiguous())):
        raise ValueError("fail uint8 [B], orig int64 [B], iters int32 [B], kind uint8 [n], sent uint8 [rows, n]")
    _lib.check(_lib.load().ldpc_harq_tally(xhat.data_ptr(), None if sent is None else sent.data_ptr(), 0 if sent is None else sent.shape[0], int(codeword),
                                           kind.data_ptr(), None if iters is None else iters.data_ptr(), fail.data_ptr(),
                                           None if orig is None else orig.data_ptr(), B, n, int(hist_bins), int(t), int(T), int(tx_bits),
                                           counters.data_ptr(), torch.cuda.current_stream(counters.device).cuda_stream))


class HarqHandle:
    """An incremental-redundancy schedule (``ratematch.Harq``) around the handle of an LLR decoder: ``simulate`` in the call shape of
    ``DecoderHandle.simulate`` with ``extra_counters = T + 2`` more words behind the histogram (``ack[T]``, ``undetected``, ``sym``).  Per
    chunk of ``inner.words_chunk(channel)`` frames: the sent words as ``PatternHandle.sent_words`` makes them, then for
    ``t = 0 .. T - 1`` while rows remain: ``ldpc_harq_transmit`` (old soft buffer -> new, gathering the surviving rows) -> the inner
    handle's ``decode_device(priors, None, ..)`` -> ``ldpc_harq_syndrome`` -> ``ldpc_harq_tally`` -> the ascending list of the failing rows.
    ``y0`` is None on both channels: a combined buffer has no received word to check at iteration 0.  The length of the survivor list is
    read on the host once per transmission and chunk -- the next decode needs its batch size.

    Served: ``DecoderHandle`` (SPA, MSA, NMSA, QMSA, LMSA), ``LqmsaHandle``, ``QcHandle``, ``SlqHandle``.  Refused (ValueError, before any
    device call): everything ``PatternHandle`` refuses, and ``OsdHandle``, whose output is always a codeword."""
    CHUNK = None  # frames per chunk; None: ``inner.words_chunk(channel)`` (a test forces a small one here)

    def __init__(self, inner, harq, short_llr=32.0):
        if isinstance(inner, OsdHandle):
            raise ValueError("OSD always returns a codeword, so the acknowledgement rule (a satisfied syndrome) never asks for a retransmission")
        self.words = PatternHandle(inner, harq.pattern, short_llr)  # its refusals; the pattern on the device and the sent words
        self.inner, self.harq, self.pattern, self.short_llr = inner, harq, harq.pattern, self.words.short_llr
        self.code, self.device, self.precision = self.words.code, self.words.device, self.words.precision
        self.extra_counters = harq.T + 2

    def tables_device(self):
        """``harq.cnt`` and ``harq.first`` as CUDA uint8 tensors [T, n] on the handle's device, kept on the handle."""
        import torch

        if getattr(self, "_tables", None) is None:
            dev = torch.device("cuda", self.device)
            self._tables = (torch.from_numpy(self.harq.cnt).to(dev), torch.from_numpy(self.harq.first).to(dev))
        return self._tables

    def simulate(self, channel, param, codeword, seed, stream_id, frame0, B, max_iter, counters, flags=0, hist_bins=0):
        """Same call shape as DecoderHandle.simulate; ``counters`` (CUDA int64 [4 + hist_bins + T + 2]) is accumulated into.  TOT / WEC / BEC
        count FRAMES (once, when they leave); ITER_SUM and the histogram count decode attempts."""
        import torch

        check_pattern_run(channel, prior_grid=_lib.prior_grid_of_flags(flags))
        codeword = int(codeword)
        if codeword not in (-1, 0, 1):
            raise ValueError("codeword is 0, 1 or -1 (a random codeword per frame)")
        if codeword == 1 and self.pattern.shortened.size:
            raise ValueError("the all-one word is no codeword of the shortened code")
        if not 0 <= int(stream_id) < 65536:
            raise ValueError("stream_id below 65536: the copy ordinal lives in bits 16 and up of the stream word")
        if B <= 0:
            return
        harq, T, kind = self.harq, self.harq.T, self.words.kind_device()
        cnt, first = self.tables_device()
        chunk = int(self.CHUNK or self.inner.words_chunk(channel))
        last = int(frame0) + int(B)
        for start in range(int(frame0), last, chunk):
            rows = min(chunk, last - start)
            sent = self.words.sent_words(seed, stream_id, start, rows) if codeword == -1 else self.words.ones_words(rows) if codeword == 1 else None
            src = orig = soft = None
            for t in range(T):
                soft = harq_transmit(channel, self.precision, param, sent, 0, kind, cnt[t], first[t], self.short_llr, seed, stream_id, start,
                                     rows, src, orig, soft)
                xhat, iters = self.inner.decode_device(soft, None, max_iter, flags)[:2]
                fail = harq_syndrome(self.inner.code_handle, xhat)
                harq_tally(xhat, sent, 0, kind, iters, fail, orig, hist_bins, t, T, harq.tx_bits[t], counters)
                if t == T - 1:
                    break
                src = torch.nonzero(fail).squeeze(1)  # ascending
                rows = int(src.shape[0])  # the one host read per transmission and chunk
                if rows == 0:
                    break
                orig = src if orig is None else orig[src]
