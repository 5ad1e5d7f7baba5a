"""CAMO_FWD_FUSED_MAPS in the launch plan, pinned on the CPU (camo_debug_plan; the table of the calls without the flag is
tests/test_schedule_plan.py's).

The flag is a permission: an inference call that wants attention maps may take the fused row-tile schedule and produce them with
one launch behind the back half (csrc/attn_maps.hip).  That launch reads Q16 / Q2_16 / KV16 / KV2_16 and lse2 from the workspace,
so such a plan has a front half that writes them (the 32-row one below 10 240 packed rows, the wide one from there on while the
largest sample fits its tiles: 2944 rows at two tiles per block, below 28 672 packed rows) and the 32-row back half.  The
expected plans are literals written from that rule (include/camo_fusion.h), not read off make_plan.  Everywhere the flag may not
take effect, the plan must equal, byte for byte, the plan of the same call without it.
"""
import ctypes as C

import pytest

from camouflage_multimodal_amd import _lib
from test_schedule_plan import KINDS, REF, describe

FUSED_MAPS = getattr(_lib, "FWD_FUSED_MAPS", None)


def plan(B, T, Nk=13, max_nr=None, kind="infer", prec=_lib.PREC_BF16, attn=1, fused_maps=1, proj=3, dims=None, cus=256, opts=None):
    assert FUSED_MAPS == 4, "the binding has no FWD_FUSED_MAPS flag"
    o = _lib.default_options()
    for k, v in (opts or {}).items():
        setattr(o, k, v)
    d = _lib.CamoDims(dropout=0.1, options=C.pointer(o), **dict(REF, **(dims or {})))
    call_kind, flags = KINDS[kind]
    p = _lib.CamoPlan()
    flags |= (_lib.FLAG_ATTN_MAPS if attn else 0) | (FUSED_MAPS if fused_maps else 0)
    _lib.check(_lib.lib().camo_debug_plan(C.byref(d), proj, B, T, Nk, max_nr if max_nr is not None else min(T - B + 1, 600), prec,
                                          flags, call_kind, cus, C.byref(p)), "camo_debug_plan")
    return p


def line(p, kind="infer"):
    """test_schedule_plan.describe + the new field; every field the line leaves out must be 0."""
    s, used = describe(p, kind)
    if p.maps:
        s += " maps"
    used |= {"maps"}
    assert p.maps in (0, 1)
    assert all(getattr(p, n) == 0 for n in _lib.PLAN_FIELDS if n not in used), [(n, getattr(p, n)) for n in _lib.PLAN_FIELDS]
    return s


TAKES_EFFECT = [
    ("B1_T500", dict(B=1, T=500, max_nr=500), "fused shadows nosave front=rows32 back=rows32 tail=one_launch maps"),
    ("B16_T1600", dict(B=16, T=1600), "fused shadows nosave front=rows32 back=rows32 tail=one_launch maps"),
    ("B24_T10239", dict(B=24, T=10239), "fused shadows nosave front=rows32 back=rows32 tail=one_launch maps"),
    ("B24_T10240", dict(B=24, T=10240), "fused shadows nosave front=wide:2 back=rows32 tail=one_launch maps"),
    ("B96_T10239", dict(B=96, T=10239), "fused shadows nosave front=rows32 back=rows32 tail=gemms maps"),
    ("B96_T10240", dict(B=96, T=10240), "fused shadows nosave front=wide:2 back=rows32 tail=gemms maps"),
    ("B64_T28671", dict(B=64, T=28671), "fused shadows nosave front=wide:2 back=rows32 tail=gemms maps"),
    ("B64_T28672", dict(B=64, T=28672), "fused shadows nosave front=wide:4 back=rows32 tail=gemms maps"),
    ("B256_T128000", dict(B=256, T=128000), "fused shadows nosave front=wide:4 back=rows32 tail=gemms maps"),
    # the largest sample against the wide tiles' and the schedule's own limits
    ("maxnr2944_T12000", dict(B=24, T=12000, max_nr=2944), "fused shadows nosave front=wide:2 back=rows32 tail=one_launch maps"),
    ("maxnr2945_T12000", dict(B=24, T=12000, max_nr=2945), "fused shadows nosave front=rows32 back=rows32 tail=one_launch maps"),
    ("maxnr4096_T12000", dict(B=24, T=12000, max_nr=4096), "fused shadows nosave front=rows32 back=rows32 tail=one_launch maps"),
    ("maxnr4096_T60000", dict(B=24, T=60000, max_nr=4096), "fused shadows nosave front=wide:4 back=rows32 tail=one_launch maps"),
    ("Nk16_T1600", dict(B=16, T=1600, Nk=16), "fused shadows nosave front=rows32 back=rows32 tail=one_launch maps"),
    ("Nk1_T1600", dict(B=16, T=1600, Nk=1), "fused shadows nosave front=rows32 back=rows32 tail=one_launch maps"),
    # one map pointer is a map request like two (camo_debug_plan sees one bit either way); a device too small for the one-launch tail
    ("B16_T1600_cus48", dict(B=16, T=1600, cus=48), "fused shadows nosave front=rows32 back=rows32 tail=gemms maps"),
]


@pytest.mark.parametrize("name,args,want", TAKES_EFFECT, ids=[c[0] for c in TAKES_EFFECT])
def test_flag_plans_fused_with_a_front_half_that_writes_q16(name, args, want):
    p = plan(**args)
    assert line(p) == want
    # the maps launch's inputs: a front launch of both streams (not the KG rows' alone) and the back half that stores lse2
    assert p.nodes == 3 and p.maps == 1 and p.front in (0, 1) and p.back == 0 and p.shadows == 1 and p.save == 0
    # without the flag the same call plans what it plans today
    assert line(plan(fused_maps=0, **args)) in ("bf16", "general")


NO_EFFECT = [
    ("save_call", dict(B=16, T=1600, kind="save")),                      # not an inference call
    ("save_call_large", dict(B=24, T=12000, kind="save")),
    ("backward", dict(B=16, T=1600, kind="backward")),
    ("train", dict(B=16, T=1600, kind="train")),
    ("f32", dict(B=16, T=1600, prec=_lib.PREC_F32)),
    ("late", dict(B=16, T=1600, dims=dict(fusion_type=_lib.FUSION_LATE))),
    ("hidden128", dict(B=16, T=1600, dims=dict(hidden_dim=128))),
    ("heads4", dict(B=16, T=1600, dims=dict(num_heads=4))),
    ("rg_dim64", dict(B=16, T=1600, dims=dict(rg_dim=64))),
    ("no_rg_proj", dict(B=16, T=1600, proj=2)),
    ("maxnr4097", dict(B=24, T=12000, max_nr=4097)),
    ("maxnr4097_large", dict(B=24, T=60000, max_nr=4097)),
    ("Nk17", dict(B=16, T=1600, Nk=17)),
    ("fused_off", dict(B=16, T=1600, opts=dict(fused=0))),
]


@pytest.mark.parametrize("name,args", NO_EFFECT, ids=[c[0] for c in NO_EFFECT])
def test_flag_without_effect_changes_nothing(name, args):
    a, b = plan(fused_maps=1, **args), plan(fused_maps=0, **args)
    assert bytes(a) == bytes(b) and a.maps == 0
    kind = args.get("kind", "infer")
    if kind in ("infer", "save"):
        assert a.nodes != 3, "a map request without the permission never takes the fused schedule"


@pytest.mark.parametrize("B,T", [(1, 500), (16, 1600), (24, 10239), (24, 10240), (96, 28672), (256, 128000)])
def test_flag_without_a_map_request_is_the_plain_inference_plan(B, T):
    a, b = plan(B, T, attn=0, fused_maps=1), plan(B, T, attn=0, fused_maps=0)
    assert bytes(a) == bytes(b) and a.maps == 0 and a.nodes == 3


def test_abi_version_and_binding():
    import os
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "camo_fusion.h")).read()
    assert "#define CAMO_FWD_FUSED_MAPS 4" in hdr and _lib.FWD_FUSED_MAPS == 4
    assert _lib.ABI_VERSION >= 12 and _lib.PLAN_FIELDS[-1] == "maps"
    assert C.sizeof(_lib.CamoPlan) == 4 * len(_lib.PLAN_FIELDS)
