"""ldpc_decoder_create against the package's registry: every algorithm x storage type x backend is accepted or refused as the facts of
ldpc_decoders_amd/registry.py predict -- the library's table (kAlgs) and the package's say the same.  Create only, no decode."""
import ctypes

import pytest

pytestmark = pytest.mark.gpu

OK, E_ARG, E_UNSUPPORTED = 0, -1, -4  # include/ldpc_hip.h


def _predicted(alg, dtype, backend):
    from ldpc_decoders_amd import registry

    if alg == "BEC":  # the erasure decoder behind bec.SPA / bec.MSA: integer arithmetic, no fp16 storage (main.test refuses f16 over the bec)
        f16, streaming_only = False, False
    else:
        row = registry.BY_NAME[alg]
        f16, streaming_only = row.f16, row.refuses_fused
    if streaming_only:  # runs on the streaming kernels in fp32 / fp64: the other requests name something that does not exist
        return E_UNSUPPORTED if (dtype == "f16" or backend == "fused") else OK
    if dtype == "f16" and (not f16 or backend == "fused"):  # fp16 storage is the streaming kernels'
        return E_ARG
    return OK  # (the code below has an LDS-resident shape for every algorithm that has any)


def test_create_accepts_what_the_registry_says_exists():
    from ldpc_decoders_amd import _lib, codes
    from ldpc_decoders_amd._device import CodeHandle

    lib = _lib.load()
    code = CodeHandle(codes.get_code("512_3_6_rand_ldpc_1"), 0)  # the smallest shipped code with an LDS-resident shape
    got, want = {}, {}
    for alg in _lib.ALG:
        for dtype in _lib.DTYPE:
            for backend in _lib.BACKEND:
                h = ctypes.c_void_p()
                rc = lib.ldpc_decoder_create(code.h, _lib.ALG[alg], _lib.DTYPE[dtype], _lib.BACKEND[backend], ctypes.byref(h))
                if rc == OK:
                    assert h.value
                    _lib.check(lib.ldpc_decoder_destroy(h))
                got[alg, dtype, backend], want[alg, dtype, backend] = rc, _predicted(alg, dtype, backend)
    assert sorted(_lib.ALG.values()) == list(range(len(_lib.ALG)))  # every row of the library's table
    assert lib.ldpc_decoder_create(code.h, len(_lib.ALG), 0, 0, ctypes.byref(ctypes.c_void_p())) == E_ARG  # and no row beyond them
    assert got == want, {k: (got[k], want[k]) for k in got if got[k] != want[k]}
