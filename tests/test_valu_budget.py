"""tools/valu_budget.py on the built tree (no GPU: it cross-compiles for gfx950 and counts instructions in the assembly): every
range-specialised function of bayesssm_amd/csrc/fastmath.hip.h must take fewer vector instructions than the library form it
replaces, so that a change which brings the library's guards back in is caught."""
import tools.valu_budget as vb


def test_specialised_forms_take_fewer_vector_instructions():
    res = vb.budget()
    checked = 0
    for lib, fast in vb.PAIRS:
        if fast is None:
            continue
        assert lib in res and fast in res, (lib, fast, sorted(res))
        for key in ("valu", "valu_no_mov"):
            assert 0 < res[fast][key] < res[lib][key], (fast, key, res[fast], res[lib])
        assert res[fast]["f64_trans"] <= res[lib]["f64_trans"]
        checked += 1
    assert checked == 4


def test_a_body_with_a_branch_is_refused():
    import pytest
    asm = "vb_f:\n\tv_add_f64 v[0:1], v[0:1], v[2:3]\n\ts_cbranch_execz .LBB0_2\n\tv_mul_f64 v[0:1], v[0:1], v[0:1]\n.Lfunc_end0:\n"
    with pytest.raises(RuntimeError, match="straight-line"):
        vb.count(asm)
    assert vb.count(asm.replace("\ts_cbranch_execz .LBB0_2\n", ""))["f"]["valu"] == 2
