"""The two tables a decoder variant is stated in -- the library's (kAlgs, csrc/ldpc_common.hpp; the shape lists,
csrc/ldpc_fused_shapes.hpp) and the package's (ldpc_decoders_amd/registry.py) -- checked without a GPU."""
import ctypes

import numpy as np
import pytest

SHIPPED = ["512_3_6_rand_ldpc_1", "1200_3_6_rand_ldpc_1", "1200_rho_x5_rand_ldpc_1", "margulis"]


@pytest.mark.parametrize("name", SHIPPED)
def test_a_min_sum_variant_never_changes_the_shape(name, tmp_path):
    """A decoder takes the same LDS-resident shape, and with it the same layout plan, whether it runs plain, corrected or fixed-point
    min-sum: the tables of the variants are expanded from the list the min-sum table is.  ldpc_plan_layout is host-only."""
    from ldpc_decoders_amd import _lib, codes

    lib = _lib.load()
    code = codes.get_code(name)
    chk = np.ascontiguousarray(code.edge_chk, dtype=np.int32)
    var = np.ascontiguousarray(code.edge_var, dtype=np.int32)

    def plan(alg, dtype):
        out = tmp_path / ("%s_%s" % (alg, dtype))  # a store of its own: every call plans for itself
        out.mkdir()
        info = (ctypes.c_double * 4)()
        _lib.check(lib.ldpc_plan_layout(code.m, code.n, code.E, chk.ctypes.data, var.ctypes.data, _lib.ALG[alg], _lib.DTYPE[dtype], 2000,
                                        str(out).encode(), info))
        return list(info)

    for dtype in ("f32", "f64"):
        base = plan("MSA", dtype)
        assert base[0] > 0, (name, dtype, "no LDS-resident shape")
        for alg in ("NMSA", "QMSA"):
            assert plan(alg, dtype) == base, (name, dtype, alg)


def test_every_decoder_name_is_one_registry_row():
    from ldpc_decoders_amd import bec, biawgn, bsc, main, models, registry, utils

    choices = next(a for a in main.build_parser()._actions if a.dest == "decoder").choices
    assert list(choices) == [r.name for r in registry.ROWS] and len(set(choices)) == len(choices)
    for row in registry.ROWS:
        for mod in (biawgn, bsc):
            cls = getattr(mod, row.name)
            assert cls.__name__ in (row.name, "BiawgnML", "BscML")
            backing = row.backing.get(mod.Channel.name) if isinstance(row.backing, dict) else row.backing
            assert cls.id_keys == (backing.id_keys if backing is not None else []), (mod.__name__, row.name)
            if backing is None:
                with pytest.raises(NotImplementedError, match="outside the GPU belief-propagation path"):
                    cls(0.1, None, max_iter=1)
        cls = getattr(bec, row.name)
        if row.bec_refusal is not None:
            assert cls.id_keys == row.backing.id_keys and cls.__name__ == row.name
            with pytest.raises(NotImplementedError) as e:
                cls(0.1, None, max_iter=1)
            assert str(e.value) == row.bec_refusal[1] and "does not exist over the bec" in str(e.value)
    assert {r.name for r in registry.ROWS if r.bec_refusal is not None} == {"NMSA", "QMSA", "LMSA", "OSD"}
    assert models.decoder_names == ["ML", "SPA", "MSA", "LP", "ADMM", "ADMMA"]
    assert models.extra_decoder_names == ["NMSA"]
    assert models.fixed_point_decoder_names == ["QMSA"]
    assert models.layered_decoder_names == ["LMSA"]
    assert models.post_processing_decoder_names == ["OSD"]
    for lst in ("decoder_names", "extra_decoder_names", "fixed_point_decoder_names", "layered_decoder_names", "post_processing_decoder_names"):
        assert getattr(utils, lst) is getattr(models, lst)
    # the facts main.test looks up, as the tuples it used to carry
    have = lambda fact: [r.name for r in registry.ROWS if getattr(r, fact)]  # noqa: E731
    assert have("device_words") == ["SPA", "MSA", "NMSA", "QMSA", "LMSA", "OSD"]
    assert have("tie_dominated") == ["MSA", "NMSA", "LMSA", "OSD"]
    assert have("pops_layers") == ["LMSA", "OSD"]
    assert have("f16") == ["SPA", "MSA", "NMSA", "QMSA"]
    assert have("refuses_fused") == ["LMSA"]
    assert [r.name for r in registry.ROWS if r.prior_grid is False] == ["NMSA", "QMSA", "LMSA", "OSD"]
    assert [r.name for r in registry.ROWS if r.prior_grid is True] == ["MSA"]
    assert list(registry.osd_fronts()) == ["SPA", "MSA", "NMSA", "QMSA", "LMSA"]
