"""What the front ends share, without a GPU: rawaudiovae_kelsey_amd/frontend.py and corpus.py.

The table tests/golden/frontend_messages.json holds, for every numeric flag of every front end at the repository's root
(a word, zero, a negative number, a fraction for the integers, inf and nan for the reals), for --window, the missing
command and the limits, what parse_args(argv) raised before the front ends shared their parsing: the exception's type and
its text, or null where the flags were accepted.  It is replayed with ==.  The other tests hold the shared pieces to the
exact sentences their separate copies raised, and the three .npz codecs to the layout their docstrings state."""
import argparse
import importlib
import json
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from conftest import GOLDEN, REPO  # noqa: E402

sys.path.insert(0, REPO)

from rawaudiovae_kelsey_amd import corpus as C  # noqa: E402
from rawaudiovae_kelsey_amd import frontend as F  # noqa: E402

with open(os.path.join(GOLDEN, "frontend_messages.json")) as _f:
    TABLE = json.load(_f)


def test_the_table_covers_every_front_end():
    assert len(TABLE) == 438
    assert {e["script"] for e in TABLE} == {"interpolate", "som", "resynth", "mosaic", "evaluate", "latent_pca", "generate",
                                            "align", "segment", "restore", "recur", "states"}
    assert sum(e["error"] is not None for e in TABLE) == 399


@pytest.mark.parametrize("script", sorted({e["script"] for e in TABLE}))
def test_parse_args_raises_what_it_raised(script, monkeypatch):
    monkeypatch.chdir(REPO)        # `--audio .` and `--corpus .` name a folder
    cli = importlib.import_module(script)
    for e in (e for e in TABLE if e["script"] == script):
        try:
            cli.parse_args(list(e["argv"]))
            got = (None, None)
        except BaseException as err:      # SystemExit included: argparse's own refusals are part of the record
            got = (type(err).__name__, str(err))
        assert got == (e["error"], e["text"]), e["argv"]


def test_number_flag_spells_the_flag_with_dashes_and_the_attribute_without():
    args = argparse.Namespace(detect_zeros="0", fade=None, noise="nan", sigma="2.5")
    with pytest.raises(ValueError) as e:
        F.positive_int(args, "detect-zeros")
    assert str(e.value) == "--detect-zeros '0': expected a positive integer"
    args.detect_zeros = "64"
    assert F.positive_int(args, "detect-zeros") == 64 and args.detect_zeros == 64
    assert F.nonneg_int(args, "fade") is None and args.fade is None
    with pytest.raises(ValueError) as e:
        F.number_flag(args, "fade", int, lambda x: x >= 0, "a non-negative integer", none_ok=False)
    assert str(e.value) == "--fade None: expected a non-negative integer"
    with pytest.raises(ValueError) as e:
        F.number_flag(args, "noise", float, F.finite(1e-8, 1e8), "a finite number in [1e-8, 1e8]")
    assert str(e.value) == "--noise 'nan': expected a finite number in [1e-8, 1e8]"
    assert F.positive_real(args, "sigma") == 2.5
    for value, text in (("inf", "--sigma 'inf': expected a finite number >= 0"), ("-0.5", "--sigma '-0.5': expected a finite number >= 0")):
        args.sigma = value
        with pytest.raises(ValueError) as e:
            F.nonneg_real(args, "sigma")
        assert str(e.value) == text
    args.window = "hamming"
    with pytest.raises(ValueError) as e:
        F.window_flag(args)
    assert str(e.value) == "--window 'hamming': expected none or hann"
    args.window = "none"
    assert F.window_flag(args) is None and args.window is None
    with pytest.raises(ValueError) as e:
        F.flagged("--a / --b", lambda: C.check_hop(16, 32, 64))
    assert str(e.value).startswith("--a / --b: hop 32: the walk was")


ASCENDING, NOT_DESCENDING = "row_start must be ascending: ", "row_start must not descend: "


def test_check_row_start_in_both_modes():
    for empty_files in (False, True):
        for rs, text in (([0, 8], "row_start must run from 0 to T=9, got 0 .. 8"),
                         ([1, 9], "row_start must run from 0 to T=9, got 1 .. 9"),
                         (np.array([0.0, 9.0]), "row_start must be a 1-D integer sequence of n_files + 1 entries, got float64 (2,)"),
                         ([9], "row_start must be a 1-D integer sequence of n_files + 1 entries, got int64 (1,)"),
                         ([0, 5, 3, 9], (NOT_DESCENDING if empty_files else ASCENDING) + "file 1 is [5, 3)")):
            with pytest.raises(ValueError) as e:
                C.check_row_start(rs, 9, empty_files)
            assert str(e.value) == text
    with pytest.raises(ValueError) as e:
        C.check_row_start([0, 3, 3, 9], 9)                    # an empty file in the middle
    assert str(e.value) == ASCENDING + "file 1 is [3, 3)"
    assert C.check_row_start([0, 3, 3, 9], 9, empty_files=True).tolist() == [0, 3, 3, 9]
    assert C.check_row_start([0, 0, 9, 9], 9, empty_files=True).tolist() == [0, 0, 9, 9]
    given = np.array([0, 4, 9], dtype=np.int64)
    given.setflags(write=False)
    for empty_files in (False, True):
        got = C.check_row_start(given, 9, empty_files)
        assert got.dtype == np.int64 and got.flags.writeable and got.flags.c_contiguous and not np.shares_memory(got, given)
        got[1] = 5
        assert given.tolist() == [0, 4, 9]
        got = C.check_row_start(torch.tensor([0, 4, 9], dtype=torch.int32), 9, empty_files)
        assert got.dtype == np.int64 and got.tolist() == [0, 4, 9]


WALK_UNIT, STATES_UNIT = "one step of the walk is one frame at that hop", "a transition is one frame at that hop"


def test_check_hop_with_each_pair_of_phrases():
    import states as cli
    assert cli.HOP_PHRASES == ("the states were", STATES_UNIT)
    for phrases, text in (((), "hop 32: the walk was fitted at hop 16; " + WALK_UNIT),
                          (cli.HOP_PHRASES, "hop 32: the states were fitted at hop 16; " + STATES_UNIT),
                          (("the axes were", STATES_UNIT), "hop 32: the axes were fitted at hop 16; " + STATES_UNIT)):
        assert C.check_hop(16, 16, 64, *phrases) == 16 and C.check_hop(None, None, 64, *phrases) == 64
        assert C.check_hop(None, 64, 64, *phrases) == 64 and C.check_hop(64, None, 64, *phrases) == 64
        with pytest.raises(ValueError) as e:
            C.check_hop(16, 32, 64, *phrases)
        assert str(e.value) == text
        with pytest.raises(ValueError) as e:
            C.check_hop(16, None, 64, *phrases)
        assert str(e.value) == text.replace("hop 32", "hop 64")
        meta, cfg = dict(segment_length=64, latent_dim=8, hop=16), dict(segment_length=64, latent_dim=8)
        assert F.check_fitted("pca", "p.npz", meta, cfg) is None and F.check_fitted("pca", "p.npz", meta, cfg, 16, *phrases) == 16
        with pytest.raises(ValueError) as e:
            F.check_fitted("pca", "p.npz", meta, cfg, 32, *phrases)
        assert str(e.value) == "--hop: %s (--pca 'p.npz')" % text
    with pytest.raises(ValueError) as e:
        F.check_fitted("walk", "w.npz", dict(segment_length=64, latent_dim=8, hop=16), dict(segment_length=128, latent_dim=4), 32)
    assert str(e.value) == "--walk 'w.npz': fitted for segment_length 64 and latent_dim 8, the model has 128 and 4"
    with pytest.raises(ValueError) as e:
        F.check_exists("states", "none.npz")
    assert str(e.value) == "--states 'none.npz': no such file"


L, K, N_STATES = 4, 2, 3
I8, F8 = np.dtype(np.int64), np.dtype(np.float64)


def _t(*shape):
    return torch.from_numpy(np.random.default_rng(sum(shape)).uniform(0.5, 2, shape))


def _pca():
    from rawaudiovae_kelsey_amd import pca as P
    return P.LatentPCA(K)._set(_t(L), _t(L, L), torch.tensor([4.0, 3.0, 2.0, 1.0], dtype=torch.float64), 10, 3, K)


def _walk(mode="full"):
    from rawaudiovae_kelsey_amd import walk as W
    return W.LatentWalk(K, mode)._set(_t(L), _t(K, L), _t(K), _t(2, K, K), _t(K, L), _t(K, L) + 1, 3, 10, 2)


def _states():
    from rawaudiovae_kelsey_amd import states as ST
    theta = ST.pack_theta(np.arange(6.0).reshape(N_STATES, K), np.ones((N_STATES, K)), np.full(N_STATES, 1 / 3),
                          np.full((N_STATES, N_STATES), 1 / 3))
    return ST.LatentStates(N_STATES, K, 2e-3)._set(torch.from_numpy(theta), _t(L), _t(K, L), 10, 2, [-10.5, -9.25])


def _layout(path):
    with np.load(path) as z:
        return {n: (z[n].dtype, z[n].shape) for n in z.files}


def test_the_three_files_keep_their_layout_and_round_trip(tmp_path):
    from rawaudiovae_kelsey_amd import pca as P
    from rawaudiovae_kelsey_amd import states as ST
    from rawaudiovae_kelsey_amd import walk as W
    path = str(tmp_path / "f.npz")
    pca = _pca()
    P.write_pca(path, pca, 64, 16)
    # write_pca: mean [L], components [k, L], variances [L] (every eigenvalue), all fp64, and five integers
    assert _layout(path) == dict(mean=(F8, (L,)), components=(F8, (K, L)), variances=(F8, (L,)), segment_length=(I8, ()),
                                 latent_dim=(I8, ()), hop=(I8, ()), n_frames=(I8, ()), sweeps=(I8, ()))
    back, meta = P.read_pca(path, "cpu")
    assert meta == dict(segment_length=64, latent_dim=L, hop=16, n_frames=10)
    assert (back.sweeps_, back.n_frames_, back.n_components) == (3, 10, K)
    for name in ("mean_", "components_", "explained_variance_", "all_variances_"):
        assert getattr(back, name).dtype == torch.float64 and torch.equal(getattr(back, name), getattr(pca, name)), name
    P.write_pca(path, pca, 64)
    assert int(np.load(path)["hop"]) == -1 and P.read_pca(path, "cpu")[1]["hop"] is None

    for mode in W.MODES:
        walk = _walk(mode)
        W.write_walk(path, walk, 64, 16)
        # write_walk: mean [L], components [k, L], variances [k], dynamics [2, k, k], whiten and unwhiten [k, L], fp64
        assert _layout(path) == dict(mean=(F8, (L,)), components=(F8, (K, L)), variances=(F8, (K,)), dynamics=(F8, (2, K, K)),
                                     whiten=(F8, (K, L)), unwhiten=(F8, (K, L)), segment_length=(I8, ()), latent_dim=(I8, ()),
                                     hop=(I8, ()), n_frames=(I8, ()), n_files=(I8, ()), rank=(I8, ()), diagonal=(I8, ()))
        assert int(np.load(path)["diagonal"]) == (mode == "diagonal")
        back, meta = W.read_walk(path, "cpu")
        assert meta == dict(segment_length=64, latent_dim=L, hop=16, n_frames=10, n_files=2)
        assert (back.mode, back.rank_, back.n_components) == (mode, 3, K)
        for name in ("mean_", "components_", "explained_variance_", "dyn_", "P_", "R_"):
            assert getattr(back, name).dtype == torch.float64 and torch.equal(getattr(back, name), getattr(walk, name)), name
    W.write_walk(path, walk, 64)
    assert int(np.load(path)["hop"]) == -1 and W.read_walk(path, "cpu")[1]["hop"] is None

    st = _states()
    n_theta = ST.theta_layout(N_STATES, K)[1]
    ST.write_states(path, st, 64, 16)
    # write_states: theta, mean [L] and whiten [k, L], all fp64, var_floor, ll_history, and eight integers
    assert _layout(path) == dict(theta=(F8, (n_theta,)), mean=(F8, (L,)), whiten=(F8, (K, L)), var_floor=(F8, ()),
                                 ll_history=(F8, (2,)), segment_length=(I8, ()), latent_dim=(I8, ()), hop=(I8, ()),
                                 n_frames=(I8, ()), n_files=(I8, ()), n_states=(I8, ()), n_components=(I8, ()),
                                 n_iter=(I8, ()))
    back, meta = ST.read_states(path, "cpu")
    assert meta == dict(segment_length=64, latent_dim=L, hop=16, n_frames=10, n_files=2, n_iter=2)
    assert (back.n_states, back.n_components, back.var_floor, back.ll_history_) == (N_STATES, K, 2e-3, [-10.5, -9.25])
    for name in ("theta_", "mean_", "P_"):
        assert getattr(back, name).dtype == torch.float64 and torch.equal(getattr(back, name), getattr(st, name)), name
    ST.write_states(path, st, 64)
    assert int(np.load(path)["hop"]) == -1 and ST.read_states(path, "cpu")[1]["hop"] is None


def test_a_file_that_lacks_a_key_is_refused_by_its_kind(tmp_path):
    from rawaudiovae_kelsey_amd import pca as P
    from rawaudiovae_kelsey_amd import states as ST
    from rawaudiovae_kelsey_amd import walk as W
    path = str(tmp_path / "f.npz")
    for write, read, fitted, kind, gone in ((P.write_pca, P.read_pca, _pca(), "PCA", ("components", "sweeps")),
                                            (W.write_walk, W.read_walk, _walk(), "walk", ("unwhiten", "rank", "diagonal")),
                                            (ST.write_states, ST.read_states, _states(), "states", ("whiten", "ll_history"))):
        write(path, fitted, 64, 16)
        with np.load(path) as z:
            arrays = {n: z[n] for n in z.files}
        for n in gone:
            np.savez(path, **{k: v for k, v in arrays.items() if k != n})
            with pytest.raises(ValueError) as e:
                read(path, "cpu")
            assert str(e.value) == "%s: not a latent-%s file, it lacks %s" % (path, kind, n)
        np.savez(path, **{k: v for k, v in arrays.items() if k not in ("mean", "hop")})
        with pytest.raises(ValueError) as e:
            read(path, "cpu")
        assert str(e.value) == "%s: not a latent-%s file, it lacks mean, hop" % (path, kind)
    # the shared reader on its own: fp64 contiguous arrays, integers with hop -1 -> None, the extras as they are
    np.savez(path, a=np.arange(6, dtype=np.float32).reshape(2, 3).T, hop=-1, n=7, note=np.array([1.5]))
    arrays, meta, extra = C.read_fitted(path, "test", ("a",), ("hop", "n"), ("note",))
    assert arrays["a"].dtype == np.float64 and arrays["a"].flags.c_contiguous and arrays["a"].shape == (3, 2)
    assert meta == dict(hop=None, n=7) and extra["note"].tolist() == [1.5]


def test_rows_keeps_each_callers_sentence():
    x = torch.zeros(3, 4)
    for call, text in ((lambda: C.rows(x), "x must be a 2-D float32 device tensor, got torch.float32 (3, 4) on cpu"),
                       (lambda: C.rows(x, "cov", torch.float64), "cov must be a 2-D float64 device tensor, got torch.float32 (3, 4) on cpu"),
                       (lambda: C.rows(x, "w", wording="an [N, L]"), "w must be an [N, L] float32 device tensor, got torch.float32 (3, 4) on cpu"),
                       (lambda: C.rows([1.0], "q", empty_ok=True), "q must be a 2-D float32 device tensor, got list")):
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == text
