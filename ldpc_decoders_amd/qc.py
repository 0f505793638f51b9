"""Quasi-cyclic codes and their shift-addressed layered fixed-point min-sum decoder (no upstream counterpart: the reference generates
unstructured ensembles only, src/codes.py:108-120).

H is an ``mb x nb`` array of ``Z x Z`` blocks given by a base matrix of shifts: ``-1`` is a zero block, ``0 <= s < Z`` a cyclically
shifted identity with a one at ``(i Z + r, j Z + (r + s) mod Z)``.  ``expand`` builds the code, ``find_structure`` finds the base again from
any H (so a code travels in the ordinary parity text format), ``rand_qc_ldpc`` draws shifts on a mask, and ``QCMSA`` decodes with every
block row one layer: ``layered.LQMSA``'s integer contract, bit for bit, on a kernel that needs no index tables; for lifting sizes up to 32
several frames share a wave (``qc_pack``).  The contract is the ``ldpc_qc_*`` block of include/ldpc_hip.h.

    python -m ldpc_decoders_amd.qc <count> <mb> <nb> <Z> [--dv 3] [--seed S] [--dir D]

writes ``<n>_qc_<mb>x<nb>_z<Z>_<i>.txt`` (a ``regular_mask`` of column weight ``dv``, girth >= 6) into $FILE_CODES_DIR or ``--dir``.
"""
import math

import numpy as np

from . import codes, layered
from ._device import QcHandle, as_code


def _base_of(base, Z):
    b = np.asarray(base)
    if b.ndim != 2 or b.dtype.kind not in "iu" or int(Z) != Z or Z < 1 or b.size == 0 or (b < -1).any() or (b >= Z).any():
        raise ValueError("a base matrix is an integer array [mb, nb] of shifts, -1 (zero block) or 0 <= s < Z, with Z >= 1")
    return b.astype(np.int64), int(Z)


def expand(base, Z):
    """The code of a base matrix: block (i, j) with shift s has its ones at (i Z + r, j Z + (r + s) mod Z).  The ``Code`` carries
    ``code.qc = (base, Z)``."""
    b, Z = _base_of(base, Z)
    i, j = np.nonzero(b >= 0)
    r = np.arange(Z)
    chk = (i[:, None] * Z + r[None, :]).ravel()
    var = (j[:, None] * Z + (r[None, :] + b[i, j][:, None]) % Z).ravel()
    code = codes.Code.from_edges(b.shape[0] * Z, b.shape[1] * Z, chk, var)
    code.qc = (b, Z)
    return code


def _structure_at(code, Z):
    """-> (base, None) or (None, (i, j)): the first block, row-major, that is neither zero nor one shifted identity.  O(E)."""
    mb, nb = code.m // Z, code.n // Z
    chk, var = np.asarray(code.edge_chk, dtype=np.int64), np.asarray(code.edge_var, dtype=np.int64)
    block = (chk // Z) * nb + var // Z
    shift = (var % Z - chk % Z) % Z
    # a block is a shifted identity iff it holds Z ones of one shift (distinct edges of one shift lie in distinct rows)
    blocks, first, count = np.unique(block, return_index=True, return_counts=True)
    of_edge = np.searchsorted(blocks, block)
    bad = count != Z
    bad[of_edge[shift != shift[first][of_edge]]] = True
    if bad.any():
        k = int(blocks[np.argmax(bad)])
        return None, (k // nb, k % nb)
    base = np.full(mb * nb, -1, dtype=np.int64)
    base[blocks] = shift[first]
    return base.reshape(mb, nb), None


def find_structure(code, Z=None):
    """-> (base, Z).  With ``Z``: ValueError unless Z divides m and n and every Z x Z block is zero or one shifted identity (the message
    names the first offending block).  ``Z=None``: the largest Z >= 2 dividing gcd(m, n) for which that holds; ValueError if there is none."""
    code = as_code(code)
    if Z is not None:
        if int(Z) != Z or Z < 1 or code.m % int(Z) or code.n % int(Z):
            raise ValueError("the lifting size Z = %r must be a positive integer dividing m = %d and n = %d" % (Z, code.m, code.n))
        base, at = _structure_at(code, int(Z))
        if base is None:
            raise ValueError("not quasi-cyclic at Z = %d: block (%d, %d) of the %d x %d base is neither zero nor one cyclically shifted identity"
                             % ((Z,) + at + (code.m // Z, code.n // Z)))
        return base, int(Z)
    g = math.gcd(code.m, code.n)
    for z in sorted((d for d in range(2, g + 1) if g % d == 0), reverse=True):
        base, _ = _structure_at(code, z)
        if base is not None:
            return base, z
    raise ValueError("no quasi-cyclic structure: for no Z >= 2 dividing gcd(m, n) = %d is every Z x Z block of H zero or a shifted identity" % g)


def regular_mask(mb, nb, dv):
    """Boolean [mb, nb] with ``dv`` ones per column on cyclic supports: column j meets block rows j, j + 1, .. j + dv - 1 (mod mb)."""
    if not 1 <= dv <= mb:
        raise ValueError("1 <= dv <= mb")
    mask = np.zeros((mb, nb), dtype=bool)
    for j in range(nb):
        mask[(j + np.arange(dv)) % mb, j] = True
    return mask


def has_4_cycle(base, Z):
    """Two block rows with two common columns whose shift differences agree mod Z close a cycle of length 4."""
    b = np.asarray(base)
    for i in range(b.shape[0]):
        for k in range(i + 1, b.shape[0]):
            both = (b[i] >= 0) & (b[k] >= 0)
            d = (b[i, both] - b[k, both]) % Z
            if np.unique(d).size != d.size:
                return True
    return False


def rand_qc_ldpc(mask, Z, rng=None, girth6=True, max_draws=20000):
    """Random quasi-cyclic code on a boolean mask [mb, nb]: a shift uniform on 0 .. Z - 1 for every nonzero entry.  With ``girth6`` a block
    column is redrawn until it closes no 4-cycle with the columns before it, and the whole base is begun again when a column finds no
    shifts; after ``max_draws`` column draws in all: ValueError (a dense 3 x 6 mask has no such shifts at Z = 5)."""
    rng = rng or np.random
    mask = np.asarray(mask, dtype=bool)
    if mask.ndim != 2 or int(Z) != Z or Z < 1:
        raise ValueError("a boolean mask [mb, nb] and a lifting size Z >= 1")
    mb, nb = mask.shape
    draws = 0
    while True:
        base = np.full((mb, nb), -1, dtype=np.int64)
        used = {}  # (i, k) -> shift differences of the columns placed so far
        j = 0
        tries = 0
        while j < nb:
            rows = np.flatnonzero(mask[:, j])
            s = rng.randint(0, Z, size=rows.size)
            draws += 1
            pairs = [((rows[a], rows[b]), int((s[a] - s[b]) % Z)) for a in range(rows.size) for b in range(a + 1, rows.size)]
            if not girth6 or all(d not in used.get(p, ()) for p, d in pairs):
                base[rows, j] = s
                for p, d in pairs:
                    used.setdefault(p, set()).add(d)
                j, tries = j + 1, 0
                continue
            tries += 1
            if draws >= max_draws:
                raise ValueError("no shifts without a 4-cycle found on this %d x %d mask at Z = %d in %d draws" % (mb, nb, Z, draws))
            if tries >= 8 * Z:  # this column has (almost) no free shifts left: begin again
                break
        if j == nb:
            return expand(base, Z)


def gen_rand_qc(args):
    """The command line: ``count`` codes on ``regular_mask(mb, nb, dv)`` in the parity text format, reloaded and reported like
    ``codes.gen_rand_ldpc`` does."""
    rng = np.random.RandomState(args.seed)
    out = []
    for i in range(args.count):
        code = rand_qc_ldpc(regular_mask(args.mb, args.nb, args.dv), args.Z, rng)
        name = "%d_qc_%dx%d_z%d_%d" % (code.n, args.mb, args.nb, args.Z, i + 1)
        path = codes.save_parity_mtx(code, name, args.dir)
        back = codes.load_parity_mtx(path)
        print(name, (back.m, back.n), "Z = %d" % find_structure(back, args.Z)[1], sorted(set(back.col_degrees().tolist())), sorted(set(back.row_degrees().tolist())))
        out.append(path)
    return out


def setup_parser():
    import argparse

    p = argparse.ArgumentParser()
    p.add_argument("count", type=int, help="number of random quasi-cyclic codes to generate")
    p.add_argument("mb", type=int, help="block rows of the base matrix")
    p.add_argument("nb", type=int, help="block columns of the base matrix")
    p.add_argument("Z", type=int, help="lifting size: every block is Z x Z")
    p.add_argument("--dv", type=int, default=3, help="ones per column of the base mask (cyclic supports)")
    p.add_argument("--seed", type=int, default=None, help="seed of the shifts")
    p.add_argument("--dir", default=None, help="output directory (default: $FILE_CODES_DIR or data/codes)")
    return p


# ---------------------------------------------------------------------------------------------------------------- the decoder
def qc_waves(frames_per_cu, Z):
    """Waves per frame (csrc/ldpc_qc.hpp qc_waves): ``layered.lqmsa_waves`` capped at the smallest of 1, 2, 4, 8 that is >= ceil(Z / 64)."""
    cap = next((w for w in (1, 2, 4) if w >= (Z + 63) // 64), 8)
    return min(layered.lqmsa_waves(frames_per_cu), cap)


def qc_pack_stride(lds_bytes_per_frame, Z):
    """Bytes from one frame slot's image to the next (csrc/ldpc_qc.hpp qc_pack_stride): the smallest multiple of 16 that is >= the frame's
    bytes and congruent to 2 Z rounded up to 16 modulo 128."""
    want, s = (2 * Z + 15) // 16 * 16 % 128, (lds_bytes_per_frame + 15) // 16 * 16
    return s + (want - s % 128) % 128


def qc_pack(Z, lds_bytes_per_frame):
    """Frames per wave (csrc/ldpc_qc.hpp qc_pack): 1 above Z = 32, else as many as the 64 lanes and one CU's LDS take."""
    if Z > 32:
        return 1
    return max(min(64 // Z, layered.LDS_BYTES // qc_pack_stride(lds_bytes_per_frame, Z)), 1)


def check_pack(P, Z, lds_bytes_per_frame):
    """What ``ldpc_qcpack_set`` accepts: 0 (the rule), 1, or P >= 2 frames whose rows fit the wave and whose images fit the LDS.  -> int"""
    if int(P) != P or P < 0:
        raise ValueError("qc_pack is 0 (the rule's pick), 1 or a number of frames per wave >= 2 (got %r)" % (P,))
    stride = qc_pack_stride(lds_bytes_per_frame, Z)
    if P >= 2 and (P * Z > 64 or P * stride > layered.LDS_BYTES):
        raise ValueError("QCMSA: %d frames per wave at Z = %d with %d bytes from frame to frame: P Z <= 64 lanes and P times those bytes <= %d of LDS are "
                         "needed (the rule picks %d)" % (P, Z, stride, layered.LDS_BYTES, qc_pack(Z, lds_bytes_per_frame)))
    return int(P)


def check_order(mb, order):
    """What ``ldpc_qc_set_order`` accepts: a permutation of 0 .. mb - 1.  -> int32 array"""
    o = np.asarray(order)
    if o.ndim != 1 or o.dtype.kind not in "iu" or not np.array_equal(np.sort(o), np.arange(mb)):
        raise ValueError("the order of the block rows is a permutation of 0 .. %d" % (mb - 1))
    return o.astype(np.int32)


def layers_of(Z, order):
    """The layer of every check that an order of the block rows means: the position of block row c // Z."""
    pos = np.empty(len(order), dtype=np.int64)
    pos[np.asarray(order)] = np.arange(len(order))
    return np.repeat(pos, Z)


def frame_bytes(code, base):
    """LDS bytes of one frame: ``layered.lqmsa_lds_bytes`` with the largest block-row degree."""
    return layered.lqmsa_lds_bytes(code.m, code.n, code.E, int((np.asarray(base) >= 0).sum(axis=1).max()))


def check_code(code, base, Z):
    """ValueError unless ``ldpc_qc_create`` takes the code (checked before the library is loaded)."""
    deg = (np.asarray(base) >= 0).sum(axis=1)
    dv = np.bincount(np.asarray(code.edge_var), minlength=code.n)
    if deg.min() < 2:
        raise ValueError("layered min-sum needs every check to have at least two variables (a block row of degree %d)" % deg.min())
    if dv.max() > layered.MAX_DV:
        raise ValueError("QCMSA: a variable of degree %d: the int16 marginals hold degrees up to %d" % (dv.max(), layered.MAX_DV))
    need = frame_bytes(code, base)
    if need > layered.LDS_BYTES:
        raise ValueError("QCMSA: a frame of a %d x %d code (largest block-row degree %d) needs %d bytes of LDS, above one CU's %d; "
                         "use LMSA (layered min-sum on the streaming kernels) for it" % (code.m, code.n, deg.max(), need, layered.LDS_BYTES))


def resolve(code, qc_lift=0):
    """-> (base, Z): ``qc_lift`` > 0 is checked against H; 0 takes ``code.qc`` where ``expand`` left it, else the largest Z that fits."""
    if qc_lift:
        return find_structure(code, qc_lift)
    if getattr(code, "qc", None) is not None:
        return code.qc
    return find_structure(code)


class QCMSA:
    """Layered fixed-point min-sum on a quasi-cyclic code: ``layered.LQMSA``'s rule and parameters with the block rows of the base matrix
    as layers, processed in ``qc_order`` (a permutation of the block rows; None: natural order).  ``qc_lift``: the lifting size Z (0:
    ``code.qc``, else detected).  ``qc_pack``: frames per wave for Z <= 32 (0: the rule ``qc_pack``; 1: one frame per workgroup); it changes
    the speed and no result, so it is no id key.  ``decode`` / ``decode_batch`` / ``last_iters`` as ``layered.LQMSA``."""
    id_keys = layered.LQMSA.id_keys + ["qc_lift"]

    def __init__(self, parity_mtx, max_iter=10, msa_bits=6, msa_frac_bits=2, msa_scale=0.8125, msa_offset=0, qc_lift=0, qc_order=None, qc_pack=0, **_):
        given = (msa_bits, msa_frac_bits, msa_scale, msa_offset)
        values = [d if v is None else v for v, d in zip(given, (6, 2, 0.8125, 0))]
        # (everything is checked before the decoder is created: a bad value never reaches the device)
        self.msa_bits, self.msa_frac_bits, self.msa_scale, self.msa_offset = layered.check_params(*values)
        if _.get("precision") == "f16" or _.get("backend") == "stream":
            raise ValueError("QCMSA is an LDS-resident integer kernel: no fp16 storage, no streaming backend (LMSA has one)")
        self.max_iter = int(max_iter)
        self.code = as_code(parity_mtx)
        self.base, self.qc_lift = resolve(self.code, int(qc_lift or 0))
        if qc_order is not None:
            qc_order = check_order(self.base.shape[0], qc_order)
        check_code(self.code, self.base, self.qc_lift)
        self.qc_pack = check_pack(qc_pack or 0, self.qc_lift, frame_bytes(self.code, self.base))
        self.precision = "f64" if _.get("precision") == "f64" else "f32"  # the type the priors are quantised in
        self.handle = QcHandle(self.code, self.qc_lift, _.get("device"), self.msa_bits, self.msa_frac_bits, self.msa_scale, self.msa_offset,
                               self.qc_pack)
        if qc_order is not None:
            self.handle.set_order(qc_order)
        self.last_iters = None

    @property
    def parity_mtx(self):
        return self.code.parity_mtx

    @property
    def layers(self):
        """The layer of every check that the handle's order of the block rows means."""
        return layers_of(self.qc_lift, self.handle.order())

    _host = layered.LQMSA._host
    decode = layered.LQMSA.decode
    decode_batch = layered.LQMSA.decode_batch


if __name__ == "__main__":
    gen_rand_qc(setup_parser().parse_args())
