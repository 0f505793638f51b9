"""Maximum-likelihood decoding over the BEC for codes without a code book -- the reference's ``bec.ML`` rule (src/bec.py:21-36,
math_utils.arg_max_rand at src/math_utils.py:72-74) by linear algebra instead of a code-book search.

Every codeword that agrees with the unerased symbols is equally likely.  The erasure decoder peels to its stopping-set exit; the
residual system  H_R x_R = H_Rbar y_Rbar  is brought to reduced row echelon form over GF(2) on the GPU (csrc/ldpc_bec_ml.hip) and the
free variables take bits of a Philox stream keyed by (seed, stream id, global frame index), so the pick is uniform over the solution
set.  ``last_nullity`` holds d per frame (2^d solutions; -1: no solution, the sent word was no codeword).  DESIGN.md section 14.
"""
import numpy as np

from ._device import BecMlHandle, as_code

LDS_BYTES = 160 * 1024  # one CU's LDS: the whole system of the worst-case frame (every bit erased) must fit
MAX_ROWS = 4096


def lds_bytes(m, n):
    """LDS one frame's system takes when every bit is erased: the rule of ldpc_bec_ml_create (csrc/ldpc_bec_ml.hpp)."""
    W, S, RP = (n + 31) // 32, (n + 32) // 32, -(-m // 64) * 64
    return 4 * (3 * W + 3 * S + S * RP)


def check_size(code):
    """ValueError unless the worst-case system of ``code`` fits one CU's LDS (checked before the library is loaded)."""
    if lds_bytes(code.m, code.n) > LDS_BYTES or -(-code.m // 64) * 64 > MAX_ROWS:
        raise ValueError("ML over the BEC by elimination: the system of a %d x %d code needs %d bytes of LDS when every bit is erased, "
                         "above the limit of one CU's 160 KiB (m * n <= 1310720 bits, at most %d checks)"
                         % (code.m, code.n, lds_bytes(code.m, code.n), MAX_ROWS))


class BecEliminationML:
    id_keys = []
    channel = "bec"

    def __init__(self, p, _code, **kwargs):
        self.param = p
        self.code = as_code(_code)
        check_size(self.code)
        self.n = self.code.n
        self.handle = BecMlHandle(self.code, kwargs.get("device"))
        self.last_iters = self.last_nullity = None

    def _host(self, y):
        import torch

        y = np.atleast_2d(np.asarray(y))
        if not (((y >= 0) & (y <= 2)).all()):
            raise ValueError("symbols must be in {0, 1, 2}")
        seed = int(np.random.randint(0, 2 ** 63, dtype=np.int64))  # one draw per call: --np-seed makes --exact runs repeatable
        yd = torch.from_numpy(np.ascontiguousarray(y, dtype=np.uint8)).to("cuda:%d" % self.handle.device)
        xhat, nul = self.handle.decode_device(yd, seed, 0, 0)
        return xhat.cpu().numpy(), nul.cpu().numpy()

    def decode(self, y):
        xhat, nul = self._host(y)
        self.last_nullity, self.last_iters = nul, np.zeros(1, dtype=np.int32)
        return xhat[0].astype(np.int64)

    def decode_batch(self, y):
        """[B,n] -> (x_hat [B,n], iters = zeros).  numpy in: the tie-break seed is one np.random draw; CUDA tensor in: one torch draw,
        everything stays on the GPU."""
        if hasattr(y, "is_cuda"):
            import torch

            seed = int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())
            xhat, self.last_nullity = self.handle.decode_device(y.contiguous(), seed, 0, 0)
            self.last_iters = torch.zeros(y.shape[0], dtype=torch.int32, device=y.device)
            return xhat, self.last_iters
        xhat, self.last_nullity = self._host(y)
        self.last_iters = np.zeros(xhat.shape[0], dtype=np.int32)
        return xhat, self.last_iters
