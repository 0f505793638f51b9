"""Systematic encoder of any code given by its parity checks: GF(2) elimination on the host, u . P on the matrix cores.

The reference encodes only through its code book (``Code.cb``, src/codes.py:11-19), which exists for the built-in toy codes alone;
``--codeword -1`` (src/main.py:38) is therefore limited upstream to those.  Here H is brought to reduced row echelon form over GF(2)
once per code (bit-packed uint64 rows, pivot = the first row that has a 1 in the column, columns left to right), which gives

  * ``parity_positions`` -- the r = rank pivot columns, ``info_positions`` -- the other k' = n - rank columns, ascending;
  * ``P`` (k' x r bits) with c[parity_positions] = u . P mod 2 and c[info_positions] = u for every u in GF(2)^k'.

``encode`` is the host statement of the map (numpy); ``encode_device`` / ``random_words`` run it on the GPU (csrc/ldpc_encode.hip:
``v_mfma_i32_32x32x32_i8`` on 0/1 bytes, int32 accumulation, ``& 1``).  ``random_words`` draws the info bits from Philox4x32-10 keyed
by (seed, stream id, global frame index), blocks 0x80000000 + j: bit t of word w of block j is info bit 128 j + 32 w + t.
"""
import ctypes

import numpy as np

from . import _lib

SIZE_LIMIT = 1 << 28  # m * n: the limit of Code.parity_mtx
PHILOX_INFO_BLOCK0 = 0x80000000


def gf2_systematic(code):
    """-> (rank, par_pos int32 [r], info_pos int32 [k'], P uint8 [k', r] in {0,1}).  Deterministic: column by column, the pivot of a
    column is the first row (in H's row order) not yet used as a pivot that has a 1 there."""
    m, n = code.m, code.n
    if m * n > SIZE_LIMIT:
        raise ValueError("GF(2) encoder: m * n = %d * %d exceeds the limit 2^28 of a dense parity matrix" % (m, n))
    W = (n + 63) // 64
    M = np.zeros((m, W), dtype=np.uint64)
    np.bitwise_xor.at(M, (code.edge_chk, code.edge_var >> 6), np.left_shift(np.uint64(1), (code.edge_var & 63).astype(np.uint64)))
    free = np.ones(m, dtype=bool)  # rows not yet used as a pivot
    piv_row, piv_col = [], []
    # forward elimination: a row that is still free is zero in every column left of the current one, so only words >= c >> 6 move
    for c in range(n):
        w, b = c >> 6, np.uint64(c & 63)
        cand = np.flatnonzero(free)
        if len(cand) == 0:
            break
        hit = cand[((M[cand, w] >> b) & np.uint64(1)).astype(bool)]
        if len(hit) == 0:
            continue
        p = hit[0]
        free[p] = False
        if len(hit) > 1:
            M[hit[1:], w:] ^= M[p, w:]
        piv_row.append(p)
        piv_col.append(c)
    # back substitution: clear each pivot column in the pivot rows above it (pivot row of column c is zero left of c)
    for i in range(len(piv_col) - 1, 0, -1):
        c, p = piv_col[i], piv_row[i]
        w, b = c >> 6, np.uint64(c & 63)
        rows = np.asarray(piv_row[:i])
        hit = rows[((M[rows, w] >> b) & np.uint64(1)).astype(bool)]
        if len(hit):
            M[hit, w:] ^= M[p, w:]
    r = len(piv_col)
    par_pos = np.asarray(piv_col, dtype=np.int32)
    is_par = np.zeros(n, dtype=bool)
    is_par[par_pos] = True
    info_pos = np.flatnonzero(~is_par).astype(np.int32)
    # row i of the reduced matrix: c[par_pos[i]] = sum_j R[i, info_pos[j]] u_j  ->  P[j, i] = R[i, info_pos[j]]
    R = M[np.asarray(piv_row, dtype=np.int64)] if r else np.zeros((0, W), dtype=np.uint64)
    bits = np.unpackbits(R.view(np.uint8), axis=1, bitorder="little")[:, :n] if r else np.zeros((0, n), dtype=np.uint8)
    P = np.ascontiguousarray(bits[:, info_pos].T)
    return r, par_pos, info_pos, P


class Encoder:
    """``Encoder(code)``: systematic form of ``code`` (see the module docstring).  Use ``Code.encoder()`` for the cached instance."""

    def __init__(self, code):
        self.code = code
        self.n = code.n
        self.rank, self.parity_positions, self.info_positions, self.P = gf2_systematic(code)
        self.k = self.n - self.rank
        self._dev = {}

    # ---- host
    def encode(self, u):
        """u [..., k] in {0,1} -> codewords [..., n] uint8 (numpy)."""
        u = np.asarray(u).astype(np.uint8) & 1
        if u.shape[-1] != self.k:
            raise ValueError("info words must have k' = %d bits" % self.k)
        c = np.zeros(u.shape[:-1] + (self.n,), dtype=np.uint8)
        c[..., self.info_positions] = u
        if self.rank:
            c[..., self.parity_positions] = ((u.astype(np.int64) @ self.P.astype(np.int64)) & 1).astype(np.uint8)
        return c

    # ---- device
    def handle(self, device=None):
        from ._device import current_device

        device = current_device() if device is None else device
        h = self._dev.get(device)
        if h is None:
            h = self._dev[device] = EncoderHandle(self, device)
        return h

    def encode_device(self, u):
        """u: CUDA uint8 tensor [B, k] in {0,1} -> CUDA uint8 tensor [B, n], the codewords (``ldpc_encode``)."""
        return self.handle(u.device.index).encode(u)

    def random_words(self, seed, stream_id, frame0, B, out=None):
        """Random codewords of frames [frame0, frame0 + B) as a CUDA uint8 tensor [B, n] (``ldpc_encode_random``)."""
        return self.handle().encode_random(seed, stream_id, frame0, B, out=out)


class EncoderHandle:
    """An ``Encoder``'s tables resident on one GPU (``ldpc_encoder_*``)."""

    def __init__(self, enc, device):
        lib = _lib.load()
        self.enc, self.device = enc, device
        h = ctypes.c_void_p()
        P = np.ascontiguousarray(enc.P, dtype=np.uint8)
        info = np.ascontiguousarray(enc.info_positions, dtype=np.int32)
        par = np.ascontiguousarray(enc.parity_positions, dtype=np.int32)
        _lib.check(lib.ldpc_encoder_create(device, enc.n, enc.k, enc.rank, info.ctypes.data, par.ctypes.data, P.ctypes.data, ctypes.byref(h)))
        self.h = h

    def __del__(self):
        try:
            if getattr(self, "h", None):
                _lib.load().ldpc_encoder_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def info(self):
        """The launch shape of the handle (``ldpc_encoder_info``): {"nt": 32-column tiles per wave of ``k_encode``, "cgroups": column groups
        of nt tiles, "kgroups": ceil(k / 128), "chunks": 8192-bit chunks of ``k_info``}."""
        out = (ctypes.c_int32 * 4)()
        _lib.check(_lib.load().ldpc_encoder_info(self.h, out))
        return dict(zip(("nt", "cgroups", "kgroups", "chunks"), (int(x) for x in out)))

    def encode(self, u, out=None):
        import torch

        if not u.is_cuda or u.dtype != torch.uint8 or not u.is_contiguous() or u.dim() != 2 or u.shape[1] != self.enc.k:
            raise ValueError("info words must be a contiguous CUDA uint8 tensor [B, %d]" % self.enc.k)
        B = u.shape[0]
        out = torch.empty((B, self.enc.n), dtype=torch.uint8, device=u.device) if out is None else out
        if B:
            st = torch.cuda.current_stream(u.device).cuda_stream
            _lib.check(_lib.load().ldpc_encode(self.h, u.data_ptr(), B, out.data_ptr(), st))
        return out

    def encode_random(self, seed, stream_id, frame0, B, out=None):
        import torch

        dev = torch.device("cuda", self.device)
        out = torch.empty((int(B), self.enc.n), dtype=torch.uint8, device=dev) if out is None else out
        if B:
            st = torch.cuda.current_stream(dev).cuda_stream
            _lib.check(_lib.load().ldpc_encode_random(self.h, int(seed), int(stream_id), int(frame0), int(B), out.data_ptr(), st))
        return out
