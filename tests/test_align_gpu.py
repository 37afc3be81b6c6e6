"""The alignment ops on the GPU (RV_ALIGN_*, csrc/align.hip, rawaudiovae_kelsey_amd/align.py, align.py) against
tests/align_oracle.py.  Everything is compared exactly: the local costs are the search's distance bit for bit
(mosaic_oracle.sq_dist), the DP is fp64 with a fixed candidate order, so the path, its length, the summary and both
costs are the oracle's own.

Shapes (Ta, Tb, L, r): the smallest that cross an edge -- single rows and columns, sizes off the 128 x 64 x 32 tile, a
band narrower than a tile and one that spans several, more than one row block, diagonals longer than the workgroup of
1024 threads -- and one case on each side of FW_DIAG_LDS = 2048, the cells of the longest diagonal up to which the DP
keeps its rolling diagonals in LDS (beyond: in the workspace), plus a banded case whose rows pass 2048 while its
diagonals stay short, so that the LDS form's index wraps.  The cost kernel has one form of row loads."""
import functools
import json
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from conftest import REPO  # noqa: E402
import align_oracle as O  # noqa: E402
from guarded import SENTINEL, guarded, guarded_flat  # noqa: E402

pytestmark = pytest.mark.gpu

FW_DIAG_LDS = 2048          # csrc/align.hip
ISSUE_CASES = [(1, 1, 1, 0), (1, 7, 3, 0), (7, 1, 3, 0), (5, 9, 3, 1), (130, 67, 33, 0), (257, 300, 64, 5), (300, 257, 70, 0),
               (1000, 1500, 64, 40), (600, 600, 256, 0)]
SWEEP_CASE = (1100, 1100, 8, 0)                                   # diagonals longer than the workgroup
LDS_SIDE, WS_SIDE = (FW_DIAG_LDS, FW_DIAG_LDS, 4, 0), (FW_DIAG_LDS + 1, FW_DIAG_LDS + 1, 4, 0)   # straddle FW_DIAG_LDS
WRAP_CASE = (2500, 2300, 4, 5)                                    # rows beyond FW_DIAG_LDS, diagonals of 11 cells
CASES = ISSUE_CASES + [SWEEP_CASE, LDS_SIDE, WS_SIDE, WRAP_CASE]
PENALTIES = (0.0, 0.5, 1e30)
MODES = {O.GLOBAL: "global", O.SUBSEQUENCE: "subsequence"}


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()     # a copy: the cached inputs are read-only


def _np(t):
    return t.detach().cpu().numpy()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


@functools.lru_cache(maxsize=None)
def _inputs(Ta, Tb, L, kind):
    make = O.random_latents if kind == "random" else O.binary_latents
    a, b = make(Ta, L, 7 * Ta + Tb), make(Tb, L, 1000 + 7 * Ta + Tb)
    a.setflags(write=False), b.setflags(write=False)
    return a, b


@functools.lru_cache(maxsize=None)
def _reference(Ta, Tb, L, r, kind):
    """(Dm, the full matrix) of the oracle for one case, computed once and left unchanged."""
    a, b = _inputs(Ta, Tb, L, kind)
    dm, full = O.local_costs(a, b, r)
    dm.setflags(write=False), full.setflags(write=False)
    return dm, full


def _run(a, b, r, mode=O.GLOBAL, penalty=0.0, dm=None):
    """COST (unless dm is given), FORWARD and BACKTRACK into guarded outputs -> dict of numpy results."""
    from rawaudiovae_kelsey_amd import align as A
    Ta, Tb = a.shape[0], b.shape[0]
    W = O.band_width(Tb, r)
    out = {}
    if dm is None:
        g = guarded(Ta, W, W, torch.float32)
        A.local_costs(_dev(a), _dev(b), r, out=g.view)
        g.assert_untouched("Dm")
        dm = g.payload()
    out["dm_dev"] = dm
    gp, gs, gc = guarded(Ta + Tb - 1, 2, 2, torch.float32), guarded_flat(4, torch.float32), guarded_flat(4, torch.float32)
    ge = guarded_flat(2 * Tb, torch.float32)
    views = (gp.view.view(torch.int32), gs.view.view(torch.int32).view(4), gc.view.view(torch.float64).view(2))
    end = ge.view.view(torch.float64).view(Tb)
    ws = A.forward(dm, Ta, Tb, r, MODES[mode], penalty, end_costs=end if mode == O.SUBSEQUENCE else None)
    A.backtrack(dm, Ta, Tb, r, ws, out=views)
    for g, name in ((gp, "path"), (gs, "summary"), (gc, "costs"), (ge, "end costs")):
        g.assert_untouched(name)
    out.update(path=_np(views[0]), choice=_np(views[1]), cost=_np(views[2]), path_dev=views[0].clone(),
               summary_dev=views[1].clone(), end_costs=_np(end) if mode == O.SUBSEQUENCE else None)
    if mode != O.SUBSEQUENCE:       # nothing writes the end-cost row of a global alignment
        assert (_np(ge.view) == SENTINEL).all()
    return out


def _same(got, want, what):
    assert np.array_equal(got["path"], want["path"]), (what, "path")
    assert got["choice"].tolist() == want["choice"].tolist(), (what, got["choice"], want["choice"])
    assert np.array_equal(_bits(got["cost"]), _bits(want["cost"])), (what, got["cost"], want["cost"])


# ---- COST ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("Ta,Tb,L,r", CASES)
def test_local_costs_are_the_searchs_distance_bit_for_bit(Ta, Tb, L, r):
    from rawaudiovae_kelsey_amd import align as A
    a, b = _inputs(Ta, Tb, L, "random")
    want, _ = _reference(Ta, Tb, L, r, "random")
    W = O.band_width(Tb, r)
    g = guarded(Ta, W, W, torch.float32)
    A.local_costs(_dev(a), _dev(b), r, out=g.view)
    g.assert_untouched("Dm")
    got = _np(g.payload())
    assert np.array_equal(_bits(got), _bits(want))                  # +inf outside [0, Tb), every slot written
    if r:
        assert np.isinf(want).any() and not np.isinf(want).all()
    again = A.local_costs(_dev(a), _dev(b), r)
    assert np.array_equal(_bits(_np(again)), _bits(got))            # two runs bit-equal
    if r == 0 and Ta <= 300:                                        # the search on the same operands agrees
        from rawaudiovae_kelsey_amd import mosaic as M
        _, d = M.knn_topk(_dev(a), _dev(b), 1)
        assert np.array_equal(_bits(_np(d)[:, 0]), _bits(got.min(1)))


# ---- FORWARD + BACKTRACK ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["random", "binary"])
@pytest.mark.parametrize("Ta,Tb,L,r", CASES)
def test_path_summary_and_costs_are_exactly_the_oracles(Ta, Tb, L, r, kind):
    if kind == "binary" and L > 70:
        L = 64                                                      # 0/1 rows tie at any L; the oracle's distances cost L
    a, b = _inputs(Ta, Tb, L, kind)
    dm, full = _reference(Ta, Tb, L, r, kind)
    dmd = None
    for p in PENALTIES:
        got = _run(a, b, r, O.GLOBAL, p, dmd)
        dmd = got["dm_dev"]
        C, step = O.forward(full, O.GLOBAL, p)
        want = O.backtrack(full, C, step, O.GLOBAL)
        _same(got, want, (Ta, Tb, L, r, kind, p))
        P = want["P"]
        print("align %s %s p=%g: P=%d cost %.17g path cost %.17g" % ((Ta, Tb, L, r), kind, p, P, *got["cost"]))
        assert got["choice"][3] == 1 and P >= max(Ta, Tb) and (got["path"][P:] == -1).all()
        if p == 0.0:
            assert _bits(got["cost"])[0] == _bits(got["cost"])[1]    # the same sum in the same order
        if p == 1e30 and Ta == Tb:
            assert np.array_equal(got["path"][:P], np.stack([np.arange(Ta)] * 2, 1))     # the diagonal, forced
    assert np.array_equal(_bits(_np(dmd)), _bits(dm))


@pytest.mark.parametrize("Ta,L", [(1, 3), (7, 3), (130, 33), (700, 16)])
def test_the_planted_warp_is_recovered(Ta, L):
    a, b, planted = O.planted_warp(Ta, L, Ta)
    Tb = b.shape[0]
    for r in (0, max(Ta, Tb), max(Ta, Tb) + 3):                     # a band that holds everything: the full matrix's path
        got = _run(a, b, r, O.GLOBAL, 0.0)
        P = int(got["choice"][0])
        assert P == planted.shape[0] and np.array_equal(got["path"][:P], planted) and (got["path"][P:] == -1).all()
        assert got["cost"].tolist() == [0.0, 0.0] and got["choice"].tolist() == [P, 0, Tb - 1, 1]
    _, full = O.local_costs(a, b, 0)
    for p in PENALTIES[1:]:
        want = O.backtrack(full, *O.forward(full, O.GLOBAL, p), O.GLOBAL)
        _same(_run(a, b, 0, O.GLOBAL, p), want, (Ta, L, p))
        _same(_run(a, b, max(Ta, Tb), O.GLOBAL, p), want, (Ta, L, p, "band"))


@pytest.mark.parametrize("Ta,Tb,L", [(130, 67, 33), (257, 300, 64)])
def test_a_band_that_holds_the_matrix_gives_the_full_matrixs_path(Ta, Tb, L):
    a, b = _inputs(Ta, Tb, L, "random")
    full = _run(a, b, 0, O.GLOBAL, 0.5)
    for r in (max(Ta, Tb), max(Ta, Tb) + 17):
        _same(_run(a, b, r, O.GLOBAL, 0.5), full, (Ta, Tb, r))


def test_a_nan_row_blocks_every_path_and_nothing_else():
    a, b = (x.copy() for x in _inputs(130, 67, 33, "random"))
    clean = _run(a, b, 0, O.GLOBAL, 0.0)
    bad = a.copy()
    bad[60] = np.nan
    for r in (0, 70):
        got = _run(bad, b, r, O.GLOBAL, 0.0)
        assert got["choice"].tolist() == [0, -1, -1, 0] and (got["path"] == -1).all()
        assert got["cost"].tolist() == [np.inf, 0.0]
    sub = _run(bad, b, 0, O.SUBSEQUENCE, 0.0)
    assert sub["choice"].tolist() == [0, -1, -1, 0] and sub["cost"].tolist() == [np.inf, 0.0]
    assert np.isinf(sub["end_costs"]).all()
    _same(_run(a, b, 0, O.GLOBAL, 0.0), clean, "the call after a blocked one")
    # a NaN row of b blocks one column: a global path cannot avoid it, a subsequence match on one side of it can
    badb = b.copy()
    badb[30] = np.nan
    assert _run(a[:20], badb, 0, O.GLOBAL, 0.0)["choice"][3] == 0
    got, want = _run(a[:20], badb, 0, O.SUBSEQUENCE, 0.0), O.align(a[:20], badb, 0, O.SUBSEQUENCE, 0.0)
    _same(got, want, "subsequence beside a NaN column")
    assert got["choice"][3] == 1 and np.array_equal(_bits(got["end_costs"]), _bits(want["end_costs"]))


# ---- subsequence ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("Ta,Tb,L", [(1, 7, 3), (7, 1, 3), (5, 9, 3), (64, 1300, 16), (130, 67, 33)])
def test_subsequence_search_equals_the_oracle(Ta, Tb, L):
    for kind in ("random", "binary"):
        a, b = _inputs(Ta, Tb, L, kind)
        for p in PENALTIES:
            got, want = _run(a, b, 0, O.SUBSEQUENCE, p), O.align(a, b, 0, O.SUBSEQUENCE, p)
            _same(got, want, (Ta, Tb, L, kind, p))
            assert np.array_equal(_bits(got["end_costs"]), _bits(want["end_costs"]))


def test_a_query_cut_from_a_recording_is_found_at_cost_zero_the_earlier_one_first():
    rec = O.random_latents(900, 16, 3)
    s, e = 411, 470
    got = _run(rec[s:e], rec, 0, O.SUBSEQUENCE, 0.0)
    assert got["choice"].tolist() == [e - s, s, e - 1, 1] and got["cost"].tolist() == [0.0, 0.0]
    assert np.array_equal(got["path"][:e - s], np.stack([np.arange(e - s), np.arange(s, e)], 1))
    twice = rec.copy()
    twice[700:700 + e - s] = rec[s:e]                               # the segment occurs again later
    got = _run(rec[s:e], twice, 0, O.SUBSEQUENCE, 0.0)
    assert got["choice"].tolist() == [e - s, s, e - 1, 1] and got["cost"].tolist() == [0.0, 0.0]
    assert got["end_costs"][e - 1] == 0.0 and got["end_costs"][700 + e - s - 1] == 0.0


# ---- WARP, determinism, capture ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("Ta,Tb,L,r,mode", [(1, 7, 3, 0, O.GLOBAL), (7, 1, 3, 0, O.GLOBAL), (257, 300, 64, 5, O.GLOBAL),
                                            (300, 257, 70, 0, O.GLOBAL), (20, 300, 8, 0, O.SUBSEQUENCE)])
def test_the_three_timelines_equal_the_oracle(Ta, Tb, L, r, mode):
    from rawaudiovae_kelsey_amd import align as A
    a, b = _inputs(Ta, Tb, L, "binary")
    got = _run(a, b, r, mode, 0.5)
    P = int(got["choice"][0])
    for name, timeline, n in (("a", O.ON_A, Ta), ("b", O.ON_B, Tb), ("path", O.ON_PATH, Ta + Tb - 1)):
        g = guarded(n, 2, 2, torch.float32)
        A.warp(got["path_dev"], got["summary_dev"], Ta, Tb, name, out=g.view.view(torch.int32))
        g.assert_untouched("idx " + name)
        idx = _np(g.view.view(torch.int32))
        assert np.array_equal(idx, O.warp(got["path"], P, Ta, Tb, timeline)), name
        if name == "a":
            assert np.array_equal(idx[:, 0], np.arange(Ta))         # every frame of a is visited
        if name == "b" and mode == O.SUBSEQUENCE:
            assert (idx[:got["choice"][1]] == -1).all() and (idx[got["choice"][2] + 1:] == -1).all()
    # not reached: every row of every timeline is (-1, -1)
    bad = a.copy()
    bad[0] = np.nan
    miss = _run(bad, b, r, mode, 0.5)
    for name in ("a", "b", "path"):
        assert (_np(A.warp(miss["path_dev"], miss["summary_dev"], Ta, Tb, name)) == -1).all()


def test_two_runs_and_a_captured_replay_are_bit_equal():
    from rawaudiovae_kelsey_amd import align as A
    for (Ta, Tb, L, r), mode in (((257, 300, 64, 5), "global"), ((1100, 1100, 8, 0), "global"), ((64, 300, 8, 0), "subsequence")):
        a, b = (_dev(x) for x in _inputs(Ta, Tb, L, "random"))
        runs = [A.align_latents(a, b, r, 0.5, mode) for _ in range(2)]
        cap = A.CapturedAlignment(Ta, Tb, L, r, 0.5, mode).capture()
        other = cap.replay(b[:Ta] if Tb >= Ta else a, b)             # other operands first: the replay reads the buffers
        assert other.P >= max(Ta, Tb) or mode == "subsequence"
        runs.append(cap.replay(a, b))
        ref = runs[0]
        for al in runs[1:]:
            assert torch.equal(al.path_rows, ref.path_rows) and torch.equal(al.summary, ref.summary)
            assert np.array_equal(_bits(_np(al.costs)), _bits(_np(ref.costs)))
            if mode == "subsequence":
                assert np.array_equal(_bits(_np(al.end_costs)), _bits(_np(ref.end_costs)))
        assert ref.reached and ref.P == int(ref.summary[0]) and ref.path.shape == (ref.P, 2)
        assert ref.normalised_cost == ref.path_cost / ref.P


def test_every_error_names_its_field_and_leaves_the_outputs_untouched():
    from rawaudiovae_kelsey_amd import _lib, align as A
    Ta, Tb, L, r = 20, 30, 8, 4
    a, b = (_dev(x) for x in _inputs(Ta, Tb, L, "random"))
    W = 2 * r + 1
    gd, gp = guarded(Ta, W, W, torch.float32), guarded(Ta + Tb - 1, 2, 2, torch.float32)
    gs, gc, gi = guarded_flat(4, torch.float32), guarded_flat(4, torch.float32), guarded(Tb, 2, 2, torch.float32)
    dm = A.local_costs(a, b, r)
    ws = torch.full((A.workspace_bytes(Ta, Tb, r),), 7, dtype=torch.uint8, device="cuda")
    base = dict(T=Ta, N=Tb, L=L, width=r, ws=ws.data_ptr(), ws_bytes=ws.numel(), lam=0.5)
    cost = dict(base, q=a.data_ptr(), c=b.data_ptr(), dist=gd.ptr)
    fwd = dict(base, dist=dm.data_ptr(), mode=_lib.ALIGN_GLOBAL)
    back = dict(base, dist=dm.data_ptr(), slot=gp.ptr, choice=gs.ptr, cost=gc.ptr)
    wrp = dict(T=Ta, N=Tb, slot=gp.ptr, choice=gs.ptr, idx=gi.ptr, mode=_lib.ALIGN_ON_B)
    bad = [(_lib.ALIGN_COST, cost, dict(T=0), "T=0"), (_lib.ALIGN_COST, cost, dict(N=0), "N=0"),
           (_lib.ALIGN_COST, cost, dict(L=0), "L=0"), (_lib.ALIGN_COST, cost, dict(L=4097), "L=4097"),
           (_lib.ALIGN_COST, cost, dict(width=-1), "band=-1"), (_lib.ALIGN_COST, cost, dict(T=3, N=40, width=2), "band=2"),
           (_lib.ALIGN_COST, cost, dict(q=None), "a is null"), (_lib.ALIGN_COST, cost, dict(c=None), "b is null"),
           (_lib.ALIGN_COST, cost, dict(dist=None), "local_costs is null"),
           (_lib.ALIGN_FORWARD, fwd, dict(mode=5), "mode=5"), (_lib.ALIGN_FORWARD, fwd, dict(mode=1), "band=4"),
           (_lib.ALIGN_FORWARD, fwd, dict(lam=-1.0), "penalty=-1"), (_lib.ALIGN_FORWARD, fwd, dict(lam=float("nan")), "penalty=nan"),
           (_lib.ALIGN_FORWARD, fwd, dict(dist=None), "local_costs is null"), (_lib.ALIGN_FORWARD, fwd, dict(ws=None), "ws is null"),
           (_lib.ALIGN_FORWARD, fwd, dict(ws_bytes=ws.numel() - 1), "ws_bytes=%d" % (ws.numel() - 1)),
           (_lib.ALIGN_BACKTRACK, back, dict(slot=None), "the path is null"),
           (_lib.ALIGN_BACKTRACK, back, dict(choice=None), "the summary is null"),
           (_lib.ALIGN_BACKTRACK, back, dict(cost=None), "path_costs is null"),
           (_lib.ALIGN_BACKTRACK, back, dict(ws_bytes=16), "ws_bytes=16"), (_lib.ALIGN_BACKTRACK, back, dict(T=-2), "T=-2"),
           (_lib.ALIGN_WARP, wrp, dict(mode=3), "mode=3"), (_lib.ALIGN_WARP, wrp, dict(idx=None), "warp_table is null"),
           (_lib.ALIGN_WARP, wrp, dict(slot=None), "the path is null"), (_lib.ALIGN_WARP, wrp, dict(N=0), "N=0")]
    for op, ok, change, what in bad:
        with pytest.raises(_lib.RvError) as e:
            _lib.lib().rv_mosaic(op, _lib.C.byref(_lib.MosaicDesc(**dict(ok, **change))), _lib.stream_ptr())
        assert what in str(e.value), (what, str(e.value))
    torch.cuda.synchronize()
    for g, name in ((gd, "Dm"), (gp, "path"), (gs, "summary"), (gc, "costs"), (gi, "idx")):
        g.assert_untouched(name)
        assert (_np(g.view) == SENTINEL).all(), name
    assert (_np(ws) == 7).all()


# ---- end to end -----------------------------------------------------------------------------------------------------

S, H, LAT, SR = 64, 32, 8, 8000        # the tiny model of tests/test_walk_gpu.py::test_generate_py_fit_then_run


def _model():
    from rawvae.model import VAE
    from rawaudiovae_kelsey_amd.synth import make_params
    m = VAE(S, H, LAT).cuda().eval()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in make_params(S, H, LAT, 0).items()})
    return m


def _waves():
    rng = np.random.default_rng(11)
    t = np.arange(2100) / SR
    return [(0.5 * np.sin(2 * np.pi * 330 * t) + 0.2 * rng.standard_normal(t.size)).astype(np.float32),
            (0.7 * rng.uniform(-1, 1, 1333)).astype(np.float32)]


def test_a_sound_morphed_with_itself_is_the_plain_interpolation_overlap_added():
    from rawaudiovae_kelsey_amd import align as A, interpolate as I, mosaic as M
    model, a = _model(), _waves()[0]
    hop = 16
    plain, warped = I.LatentInterpolator(model), A.AlignedInterpolator(model)
    n = I.frame_layout(a.size, S, hop)[0]
    eps = torch.from_numpy(np.random.RandomState(2).randn(n, LAT).astype(np.float32)).cuda()
    curve = np.array([0.0, 1.0, 0.25])
    frames = plain.curve(a, a, curve, hop=hop, eps=eps).view(n, S)
    from rawaudiovae_kelsey_amd.stream import window_values
    for window in (None, "hann"):
        w = None if window is None else torch.from_numpy(window_values(S, window)).cuda()
        want = M.ola(frames, hop, (n - 1) * hop + S, w)
        for timeline in ("a", "b", "path"):
            got = warped.curve(a, a, curve, hop=hop, window=window, timeline=timeline, eps=eps)
            assert torch.equal(got, want), (window, timeline)
    al = warped.last_alignment
    assert al.P == n and al.cost == 0.0 and torch.equal(al.path[:, 0], al.path[:, 1])
    # stepwise: each alpha's block overlap-added on its own
    alphas = [0.0, 0.5]
    eps2 = torch.cat([eps, eps])
    blocks = plain.stepwise(a, a, alphas, hop=hop, eps=eps2).view(2, n, S)
    want = torch.cat([M.ola(blk.contiguous(), hop, (n - 1) * hop + S, None) for blk in blocks])
    assert torch.equal(warped.stepwise(a, a, alphas, hop=hop, eps=eps2), want)


def test_a_sound_against_its_own_frames_repeated_resynthesises_itself():
    from rawaudiovae_kelsey_amd import align as A, interpolate as I
    from rawaudiovae_kelsey_amd.codec import FrameCodec
    model = _model()
    a = _waves()[0][:32 * S]                                        # whole frames
    reps = np.random.RandomState(4).randint(1, 4, size=32)
    b = np.concatenate([np.tile(a[f * S:(f + 1) * S], k) for f, k in enumerate(reps)])
    eps = torch.from_numpy(np.random.RandomState(5).randn(32, LAT).astype(np.float32)).cuda()
    alpha = (np.arange(32) % 2).astype(np.float32)                  # 0 or 1 per frame: a's row or its copy in b
    it = A.AlignedInterpolator(model)
    got = it.curve(a, b, alpha, timeline="a", eps=eps)
    al = it.last_alignment
    assert al.cost == 0.0 and al.P == reps.sum()
    assert np.array_equal(_np(al.path[:, 0]), np.repeat(np.arange(32), reps))
    mu, lv = I.LatentInterpolator(model).encode_audio(a)
    z = I.latent_mix(mu, lv, mu, lv, np.zeros(32, np.float32), "f32", eps=eps)["z"]
    want = FrameCodec(model).decode(z).reshape(-1)
    assert torch.equal(got, want)
    # a model whose mu is NaN (the ReLU in front of it swallows a NaN sample): no finite path, refused, no audio
    broken = _model()
    with torch.no_grad():
        broken.fc21.bias[0] = float("nan")
    with pytest.raises(A.RvError, match="cannot be aligned"):
        A.AlignedInterpolator(broken).curve(a, b, alpha, timeline="a", eps=eps)


def test_align_py_writes_what_it_prints(tmp_path, capsys):
    sys.path.insert(0, REPO)
    import align as cli
    from rawaudiovae_kelsey_amd import align as A
    from rawaudiovae_kelsey_amd import data as D
    wa, wb = _waves()[0], np.concatenate([_waves()[0][:700], _waves()[0][500:]])
    D.write_wav(tmp_path / "a.wav", wa, SR)
    D.write_wav(tmp_path / "b.wav", wb, SR)
    D.write_wav(tmp_path / "q.wav", wa[800:1200], SR)
    ini = tmp_path / "m.ini"
    ini.write_text("[audio]\nsampling_rate = %d\nsegment_length = %d\n[VAE]\nn_units = %d\nlatent_dim = %d\n" % (SR, S, H, LAT))
    ck = tmp_path / "ckpt"
    torch.save({"epoch": 0, "state_dict": _model().state_dict(), "optimizer": {}}, ck)
    common = ["--config", str(ini), "--checkpoint", str(ck), "--hop", "16"]
    two = common + ["--a", str(tmp_path / "a.wav"), "--b", str(tmp_path / "b.wav")]
    model = _model()
    a, b, q = (D.load_audio_mono(tmp_path / n, SR) for n in ("a.wav", "b.wav", "q.wav"))
    # path
    al = cli.main(["path"] + two + ["--band", "40", "--penalty", "0.25", "--out", str(tmp_path / "p.npz")])
    line = capsys.readouterr().out.strip().splitlines()[-1]
    want = A.LatentAligner(model).align(a, b, 16, 40, 0.25)
    with np.load(tmp_path / "p.npz") as z:
        assert np.array_equal(z["path"], _np(want.path)) and float(z["cost"]) == want.cost == al.cost
        assert float(z["path_cost"]) == want.path_cost and int(z["band"]) == 40 and int(z["hop"]) == 16
        assert (int(z["frames_a"]), int(z["frames_b"])) == (want.Ta, want.Tb)
    assert ("%d steps through %d x %d frames, cost %.9g, cost per step %.9g" % (
        want.P, want.Ta, want.Tb, want.cost, want.normalised_cost)) in line
    # morph
    y = cli.main(["morph"] + two + ["--window", "hann", "--alpha", "0:1", "--timeline", "b", "--seed", "3",
                                    "--out", str(tmp_path / "m.wav")])
    line = capsys.readouterr().out.strip().splitlines()[-1]
    ref = A.AlignedInterpolator(model).curve(a, b, np.array([0.0, 1.0]), hop=16, window="hann", timeline="b", seed=3)
    assert np.array_equal(y, _np(ref)) and np.isfinite(y).all() and np.abs(y).max() > 0
    assert D.load_audio_mono(tmp_path / "m.wav", SR).shape == y.shape and ("%d samples on timeline b" % y.size) in line
    # find
    rep = cli.main(["find"] + common + ["--query", str(tmp_path / "q.wav"), "--in", str(tmp_path / "a.wav"),
                                        "--out", str(tmp_path / "f.json")])
    line = capsys.readouterr().out.strip().splitlines()[-1]
    assert json.loads(line) == rep == json.loads((tmp_path / "f.json").read_text())
    m = A.LatentAligner(model).find(q, a, 16)
    assert rep["found"] and (rep["start_frame"], rep["end_frame"], rep["cost"]) == (m.start_frame, m.end_frame, m.cost)
    assert rep["start_sample"] == 16 * m.start_frame and rep["end_sample"] == 16 * m.end_frame + S
    assert rep["start_seconds"] == rep["start_sample"] / SR and abs(rep["start_sample"] - 800) <= 16
    assert np.array_equal(_bits(_np(m.end_costs)), _bits(_np(m.alignment.end_costs))) and m.end_costs.shape == (m.alignment.Tb,)
