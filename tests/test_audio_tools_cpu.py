"""The host layer the audio tools share, without a GPU: the one argument check behind LatentIndex.mosaic and
check_live_args, the roles of rv_mosaic_desc's shared slots (include/rawvae_hip.h, rawaudiovae_kelsey_amd/_lib.py), and
the rule that no module reaches into another's codec or stream through private names."""
import os
import re
import subprocess

import pytest

torch = pytest.importorskip("torch")

from conftest import REPO  # noqa: E402
import abi_slots  # noqa: E402

N_CORPUS = 40
BAD = [dict(k=0), dict(k=17), dict(k=N_CORPUS + 1), dict(mode="blend"), dict(continuity=-1.0),
       dict(continuity=float("nan")), dict(continuity=float("inf")), dict(fit=-1), dict(fit=1.5), dict(fit=True),
       dict(fit=1025), dict(gain_max=-1.0), dict(gain_max=float("inf")), dict(gain_max="loud"),
       dict(mode="decode", fit=4), dict(mode="decode", gain_max=2.0)]


def _offline(**kw):
    """LatentIndex.mosaic's checks come before anything touches the model or the device"""
    from rawaudiovae_kelsey_amd.mosaic import LatentIndex
    index = object.__new__(LatentIndex)
    index._n_frames = [N_CORPUS]
    return index.mosaic(None, **kw)


def _live(**kw):
    from rawaudiovae_kelsey_amd.mosaic import check_live_args
    return check_live_args(64, 16, N_CORPUS, 2, 32, hop=16, **kw)


def _message(call, **kw):
    with pytest.raises(ValueError) as e:
        call(**kw)
    return str(e.value)


@pytest.mark.parametrize("bad", BAD, ids=lambda b: ",".join("%s=%s" % kv for kv in b.items()))
def test_both_entry_points_raise_the_same_message(bad):
    from rawaudiovae_kelsey_amd.mosaic import check_mosaic_args
    ok = dict(k=2, n_corpus=N_CORPUS, mode="grains", continuity=0.0, fit=0, gain_max=0.0)
    want = _message(check_mosaic_args, **dict(ok, **bad))
    assert next(k for k in ("fit", "gain_max", "continuity", "mode", "k") if k in bad) in want
    assert _message(_offline, **bad) == want
    assert _message(_live, **bad) == want


def test_each_entry_point_keeps_its_own_order_of_checks():
    from rawaudiovae_kelsey_amd.mosaic import check_mosaic_args
    assert check_mosaic_args("3", N_CORPUS, "grains", "0.5", 4, 2) == (3, 0.5, 4, 2.0)
    wrong = dict(k=0, mode="blend", continuity=-1.0)
    assert _message(_offline, **wrong).startswith("continuity=")         # continuity, mode, k
    assert _message(_live, **wrong).startswith("mode ")                  # mode, k, continuity
    assert _message(_live, **dict(wrong, mode="grains")).startswith("k=")
    assert _message(_offline, **dict(wrong, fit=-1)).startswith("fit=")  # check_fit comes first on both paths
    assert _message(_live, **dict(wrong, fit=-1)).startswith("fit=")
    assert _message(_offline, mode="decode", fit=4, continuity=-1.0).startswith("fit=4")
    assert _message(_live, mode="decode", fit=4, continuity=-1.0).startswith("continuity=")
    assert _message(_live, mode="decode", fit=4, lag=-1).startswith("lag=")   # the lag's rules precede fit-with-decode


# Which slot of rv_mosaic_desc carries which role, and the role's C type: slot, then (role, type) with the slot's own
# name first.  Everything a call site or a host function knows about the sharing is in the header's unions; this table
# is the one other copy, held against them.
ROLES = [
    ("q", [("q", "const float*"), ("mu", "const float*"), ("a", "const float*")]),
    ("c", [("c", "const float*"), ("logvar", "const float*"), ("b", "const float*"), ("shifts", "const float*")]),
    ("idx", [("idx", "int*"), ("warp_table", "int*")]),
    ("dist", [("dist", "float*"), ("local_costs", "float*"), ("basis", "double*")]),
    ("src", [("src", "const float*"), ("moment", "const double*")]),
    ("width", [("width", "long"), ("fit_radius", "long"), ("band", "long")]),
    ("out", [("out", "float*"), ("result", "double*"), ("end_costs", "double*")]),
    ("next_of", [("next_of", "const int*"), ("room", "const int*")]),
    ("rows", [("rows", "long"), ("lag", "long")]),
    ("trans", [("trans", "float*"), ("gain", "float*"), ("centre", "double*")]),
    ("lam", [("lam", "float"), ("gain_max", "float"), ("dynamic_range", "float"), ("penalty", "float")]),
    ("slot", [("slot", "int*"), ("shift", "int*"), ("path", "int*")]),
    ("choice", [("choice", "int*"), ("info", "int*"), ("primed", "int*"), ("summary", "int*")]),
    ("cost", [("cost", "double*"), ("score", "double*"), ("eigenvalues", "double*"), ("state", "double*"),
              ("path_costs", "double*")]),
    ("weight", [("weight", "const float*"), ("gains", "const float*"), ("twiddles", "const float*")]),
]
FP64_ROLES = ("basis", "moment", "result", "end_costs", "centre", "cost", "score", "eigenvalues", "state", "path_costs")


def test_every_role_shares_its_slot_and_is_declared_with_its_own_type():
    from rawaudiovae_kelsey_amd._lib import MosaicDesc
    first = abi_slots.check_layout()        # 37 slots of 8 bytes; the header and ctypes hold the same members per slot
    declared = {slot[0][0]: list(slot) for slot in abi_slots.header_slots()}
    for slot, roles in ROLES:
        assert declared[slot] == roles, slot                                   # the names, their order and their types
        for role, _ in roles:
            assert getattr(MosaicDesc, role).offset == getattr(MosaicDesc, slot).offset == 8 * first.index(slot), role
    shared = {slot for slot, _ in ROLES}
    assert all(len(declared[slot]) == 1 for slot in first if slot not in shared)   # the other 22 slots have one name
    types = {role: ctype for _, roles in ROLES for role, ctype in roles}
    assert len(types) == sum(len(roles) for _, roles in ROLES)                 # a role names one slot
    assert all(types[role] in ("double*", "const double*") for role in FP64_ROLES)
    assert sorted(r for r, t in types.items() if "double" in t) == sorted(FP64_ROLES)
    # a descriptor built by role reads back under the slot's own name
    d = MosaicDesc(centre=0x1000, basis=0x2000, fit_radius=7, gain_max=2.5, lag=3, twiddles=0x3000, path_costs=0x4000)
    assert (d.trans, d.dist, d.width, d.lam, d.rows, d.weight, d.cost) == (0x1000, 0x2000, 7, 2.5, 3, 0x3000, 0x4000)


def test_new_names_compile_as_c99_and_carry_their_own_types(tmp_path):
    c = tmp_path / "c.c"
    c.write_text('#include "rawvae_hip.h"\n'
                 'int main(void) { rv_mosaic_desc d = {0}; const float* f = 0; const int* t = 0; int* i = 0;\n'
                 '  d.mu = f; d.logvar = f; d.warp_table = i; d.basis = (double*)0; d.moment = (const double*)0;\n'
                 '  d.fit_radius = 8; d.result = (double*)0; d.room = t; d.lag = 2; d.centre = (double*)0;\n'
                 '  d.gain_max = 2.f; d.shift = i; d.summary = i; d.eigenvalues = (double*)0; d.twiddles = f;\n'
                 '  return d.trans == (float*)d.centre && d.width == 8 && d.rows == 2 && d.lam == 2.f\n'
                 '         && (int)sizeof(d) == 37 * 8 ? 0 : 1; }\n')
    exe = tmp_path / "c"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), str(c), "-o", str(exe)],
                   check=True)
    assert subprocess.run([str(exe)]).returncode == 0


def test_live_fit_table_is_the_successors_then_room():
    from rawaudiovae_kelsey_amd.mosaic import live_fit_table
    room = torch.arange(10, dtype=torch.int32).view(5, 2) + 100
    succ = torch.tensor([1, 2, 2, 4, 4], dtype=torch.int32)
    for given, head in ((succ, succ), (None, torch.zeros(5, dtype=torch.int32))):
        t = live_fit_table(given, room)
        assert t.dtype == torch.int32 and t.is_contiguous() and t.shape == (15,)
        assert torch.equal(t[:5], head) and torch.equal(t[5:].view(5, 2), room)


def test_no_module_reaches_through_a_private_codec_or_stream():
    pkg = os.path.join(REPO, "rawaudiovae_kelsey_amd")
    for name in sorted(os.listdir(pkg)):
        if name.endswith(".py"):
            with open(os.path.join(pkg, name)) as f:
                found = re.findall(r".*(?:\._(?:enc|sv)\._|_enc\._|_sv\._).*", f.read())
            assert not found, (name, found)
