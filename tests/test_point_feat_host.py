"""CPU checks of ape_point_feat_bf16 (csrc/point_feat.hip): the export, and its refusals clause by clause.  Every refusal precedes the
launch and no pointer is followed, so this runs without a GPU; the values are tests/test_gpu_point_feat.py's business."""
import os
import re

import pytest

from conftest import REPO

X, EMB = 1, 2          # APE_POINT_FEAT_X, APE_POINT_FEAT_EMB


def _call(x4=0x1000, emb=0x2000, w1=0x3000, b1=0x4004, we1=0x5000, be1=0x6000, w2=0x7000, b2=0x8000, we2=0x9000, be2=0xA000, pf=0xB000,
          pfs=0xC000, m=5, parts=X | EMB, nsplit=3):
    from autoposeestimation_amd import _lib
    return _lib.lib().ape_point_feat_bf16(x4, emb, w1, b1, we1, be1, w2, b2, we2, be2, pf, pfs, m, parts, nsplit, None)


def test_the_export_is_declared_and_bound():
    from autoposeestimation_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "ape_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+ape_point_feat_bf16\s*\(", text)
    assert re.search(r"APE_POINT_FEAT_X\s*=\s*1\s*,\s*APE_POINT_FEAT_EMB\s*=\s*2", text)
    assert "ape_point_feat_bf16" in _lib.SIGNATURES and _lib.ABI_VERSION >= 21
    assert _lib.lib().ape_abi_version() == _lib.ABI_VERSION


@pytest.mark.parametrize("kw", [
    dict(nsplit=1), dict(nsplit=0),                                                   # split-bf16 only
    dict(parts=0), dict(parts=4), dict(parts=7), dict(parts=-1),                      # at least one half, no unknown bit
    dict(pf=None, pfs=None),                                                          # at least one output
    dict(m=-1), dict(m=1 << 31),                                                      # the row count
    dict(x4=None), dict(w1=None), dict(b1=None), dict(w2=None), dict(b2=None),        # the x half's operands
    dict(emb=None), dict(we1=None), dict(be1=None), dict(we2=None), dict(be2=None),   # the emb half's operands
    dict(x4=0x1004), dict(emb=0x2008), dict(w1=0x3002), dict(we1=0x5008), dict(w2=0x7004), dict(we2=0x9002),      # 16-byte accesses
    dict(be1=0x6004), dict(b2=0x8004), dict(be2=0xA008), dict(pf=0xB004), dict(pfs=0xC008)])
def test_bad_arguments_come_back_as_einval(kw):
    assert _call(**kw) == -1


def test_the_operands_of_an_unselected_half_are_not_looked_at():
    """with no rows there is nothing to launch, so what remains of a call is its argument check"""
    assert _call(m=0) == 0
    assert _call(m=0, parts=X, emb=None, we1=None, be1=None, we2=None, be2=None) == 0
    assert _call(m=0, parts=EMB, x4=None, w1=None, b1=None, w2=None, b2=None) == 0
    assert _call(m=0, pf=None) == 0 and _call(m=0, pfs=None) == 0
    assert _call(m=0, parts=X, emb=None) == 0 and _call(m=0, parts=X, x4=None, emb=0x2000) == -1
