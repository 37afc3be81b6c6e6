"""The host layer the audio tools share, without a GPU: the one argument check behind LatentIndex.mosaic and
check_live_args, the builders that name rv_mosaic_desc's reused fields (rawaudiovae_kelsey_amd/_lib.py), and the rule
that no module reaches into another's codec or stream through private names."""
import os
import re

import pytest

torch = pytest.importorskip("torch")

from conftest import REPO  # noqa: E402

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


def _set_fields(fields):
    """{name: value} of the fields MosaicDesc(**fields) leaves non-zero"""
    from rawaudiovae_kelsey_amd._lib import MosaicDesc
    d = MosaicDesc(**fields)
    return {n: getattr(d, n) for n, _ in MosaicDesc._fields_ if (bool(getattr(d, n)) if n == "live" else getattr(d, n))}


def test_field_builders_fill_the_documented_fields_and_nothing_else():
    from rawaudiovae_kelsey_amd import _lib
    room = torch.ones((5, 2), dtype=torch.int32)
    shift, gain, score = torch.zeros(3, dtype=torch.int32), torch.zeros(3), torch.zeros(3, dtype=torch.float64)
    assert _set_fields(_lib.fit_fields(room, 7, 2.5, shift, gain, score)) == dict(
        next_of=room.data_ptr(), width=7, lam=2.5, slot=shift.data_ptr(), trans=gain.data_ptr(), cost=score.data_ptr())
    assert _set_fields(_lib.fitted_fields(shift, gain)) == dict(slot=shift.data_ptr(), trans=gain.data_ptr())
    mu, logvar, table = torch.zeros((2, 4)), torch.zeros((2, 4)), torch.zeros(64)
    assert _set_fields(_lib.eval_fields(mu, logvar, table, 60.0)) == dict(
        q=mu.data_ptr(), c=logvar.data_ptr(), weight=table.data_ptr(), lam=60.0)
    assert _set_fields(_lib.eval_fields(mu, logvar)) == dict(q=mu.data_ptr(), c=logvar.data_ptr())
    assert _set_fields(_lib.eval_fields(None, None, table, 45.0)) == dict(weight=table.data_ptr(), lam=45.0)


def test_live_fit_table_is_the_successors_then_room():
    from rawaudiovae_kelsey_amd._lib import live_fit_table
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
