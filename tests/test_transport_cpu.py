"""The latent transport without a GPU: the op codes, descriptor roles and workspace sizes against the header, every argument
check of the five ops (they run before anything is launched) and of the Python wrappers, the .npz round trip and its
refusals, transfer.py's flags, and the oracle against itself (tests/transport_oracle.py): the row marginals after an
f-update, the error history at the target epsilon, a permuted and shifted copy mapped back onto its partners as epsilon
falls and back again by the reverse map, and the gap arithmetic of the exact-limit case."""
import ctypes as C
import re
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from conftest import REPO  # noqa: E402
import abi_slots  # noqa: E402
import transport_oracle as O  # noqa: E402

sys.path.insert(0, REPO)


def test_op_codes_roles_and_workspace_sizes():
    from rawaudiovae_kelsey_amd import _lib
    text = open(REPO + "/include/rawvae_hip.h").read()
    codes = dict(re.findall(r"#define (RV_OT_\w+) (\d+)", text))
    assert codes == dict(RV_OT_WHITEN="58", RV_OT_SOFTMIN="59", RV_OT_MAP="60", RV_OT_LIVE="61", RV_OT_WORKSPACE="62")
    assert (_lib.OT_WHITEN, _lib.OT_SOFTMIN, _lib.OT_MAP, _lib.OT_LIVE, _lib.OT_WORKSPACE) == (58, 59, 60, 61, 62)
    assert _lib.OT_WORKSPACE in _lib._HOST_ONLY_OPS
    assert not {_lib.OT_WHITEN, _lib.OT_SOFTMIN, _lib.OT_MAP, _lib.OT_LIVE} & _lib._HOST_ONLY_OPS
    para = text[text.index("/* ---- Latent transport"):text.index("#define RV_OT_WHITEN")]
    types = {n: ctype for slot in abi_slots.header_slots() for n, ctype in slot}
    for field, ctype in (("basis", "double*"), ("moment", "const double*"), ("result", "double*"), ("centre", "double*"),
                         ("state", "double*"), ("a", "const float*"), ("out", "float*"), ("weight", "const float*"),
                         ("info", "int*"), ("lam", "float"), ("T", "long"), ("N", "long"), ("L", "long"), ("k", "long"),
                         ("stride", "long"), ("ldo", "long"), ("ws_bytes", "long"), ("ws", "void*"),
                         ("live", "const struct rv_stream_desc*")):
        assert re.search(r"\b%s\b" % field, para), field
        assert hasattr(_lib.MosaicDesc, field) and types[field] == ctype, (field, types.get(field))
    # five distinct fp64 slots; out shares result's
    at = {n: getattr(_lib.MosaicDesc, n).offset for n in ("basis", "moment", "result", "centre", "state", "out")}
    assert len({at[n] for n in ("basis", "moment", "result", "centre", "state")}) == 5 and at["out"] == at["result"]
    assert len(abi_slots.check_layout()) == 37 and C.sizeof(_lib.MosaicDesc) == 37 * 8
    assert _lib.lib().rv_version() == 100 and not [n for n in _lib.EXPORTED if "ot_" in n or "transport" in n]
    for op in (38, 39, 42, 48, 57):     # still unassigned
        with pytest.raises(_lib.RvError, match="unknown op %d" % op):
            _lib.lib().rv_mosaic(op, C.byref(_lib.MosaicDesc()), None)
    up = lambda n: -(-n // 256) * 256   # noqa: E731
    for T, N, k in ((1, 1, 1), (130, 515, 17), (32768, 32768, 64), (4, 70000, 16), (5, 256, 3), (5, 257, 3)):
        slab, n = O.slabs(N)
        assert slab % 64 == 0 and slab >= 256 and n <= 8 and (n - 1) * slab < N <= n * slab
        d = _lib.mosaic_call(_lib.OT_WORKSPACE, T=T, N=N, k=k)
        assert d.ws_bytes == max(up(T * k * 8) + up(T * 4) + up(T * n * (4 + k) * 8), up(T * n * 2 * 8)), (T, N, k)
    assert O.slabs(256) == (256, 1) and O.slabs(257) == (256, 2) and O.slabs(515) == (256, 3) and O.slabs(2049) == (320, 7) and O.slabs(32768) == (4096, 8)


def _err(op, text, **fields):
    from rawaudiovae_kelsey_amd import _lib
    with pytest.raises(_lib.RvError) as e:
        _lib.lib().rv_mosaic(op, C.byref(_lib.MosaicDesc(**fields)), None)
    assert text in str(e.value), str(e.value)


def test_every_op_names_the_offending_field_before_it_launches():
    from rawaudiovae_kelsey_amd import _lib
    p = 0x1000     # never dereferenced: every call here fails a check
    whi = dict(T=10, k=2, L=4, stride=4, a=p, basis=p, result=p, info=p)
    sof = dict(T=10, N=7, k=2, basis=p, moment=p, centre=p, lam=0.5, result=p, ws=p, ws_bytes=1 << 24)
    mp = dict(T=10, N=7, k=2, L=4, stride=4, ldo=4, a=p, basis=p, moment=p, centre=p, lam=0.5, out=p, state=p, ws=p,
              ws_bytes=1 << 24)
    ops = (("OT_WHITEN", _lib.OT_WHITEN, whi), ("OT_SOFTMIN", _lib.OT_SOFTMIN, sof), ("OT_MAP", _lib.OT_MAP, mp),
           ("OT_WORKSPACE", _lib.OT_WORKSPACE, dict(T=10, N=7, k=2)))
    for name, op, ok in ops:
        for change, text in ((dict(T=0), "T=0 outside [1, 2^31)"), (dict(T=1 << 31), "T=2147483648 outside [1, 2^31)"),
                             (dict(k=0), "k=0 (the axes) outside [1, 64]"), (dict(k=65), "k=65 (the axes) outside [1, 64]")):
            _err(op, "rv_mosaic(%s): %s" % (name, text), **dict(ok, **change))
    for name, op, ok in ops[1:]:
        _err(op, "rv_mosaic(%s): N=0 (the columns) outside [1, 2^31)" % name, **dict(ok, N=0))
        _err(op, "rv_mosaic(%s): N=2147483648 (the columns) outside [1, 2^31)" % name, **dict(ok, N=1 << 31))
    for name, op, ok in (ops[0], ops[2]):
        for change, text in ((dict(L=1), "L=1 outside [k=2, 512]"), (dict(L=513, stride=513, ldo=513), "L=513 outside [k=2, 512]"),
                             (dict(stride=3), "stride=3 (the row pitch of x) holds no row of L=4 values"),
                             (dict(a=None), "a (the latent rows x) is null"),
                             (dict(basis=None), "basis (the whitening block) is null")):
            _err(op, "rv_mosaic(%s): %s" % (name, text), **dict(ok, **change))
    _err(_lib.OT_WHITEN, "result (y) is null", **dict(whi, result=None))
    _err(_lib.OT_WHITEN, "info is null", **dict(whi, info=None))
    for name, op, ok in ops[1:3]:
        for change, text in ((dict(lam=0.0), "lam=0 (epsilon) must be finite and positive"),
                             (dict(lam=-1.0), "lam=-1 (epsilon) must be finite and positive"),
                             (dict(lam=float("inf")), "lam=inf (epsilon) must be finite and positive"),
                             (dict(lam=float("nan")), "lam=nan (epsilon) must be finite and positive"),
                             (dict(moment=None), "moment (the columns' cloud) is null"),
                             (dict(centre=None), "centre (the potential and the log-weights) is null"),
                             (dict(ws_bytes=8), "ws_bytes=8, T=10 rows against N=7 columns of k=2 axes need"),
                             (dict(ws=None), "ws is null, T=10 rows"), (dict(ws=p + 8), "ws is not 256-byte aligned")):
            _err(op, "rv_mosaic(%s): %s" % (name, text), **dict(ok, **change))
    _err(_lib.OT_SOFTMIN, "basis (the rows' cloud) is null", **dict(sof, basis=None))
    _err(_lib.OT_SOFTMIN, "result is null", **dict(sof, result=None))
    _err(_lib.OT_MAP, "ldo=3 holds no row of L=4 values", **dict(mp, ldo=3))
    _err(_lib.OT_MAP, "out is null", **dict(mp, out=None))
    _err(_lib.OT_MAP, "state (the diagnostics) is null", **dict(mp, state=None))
    _err(_lib.OT_LIVE, "rv_mosaic(OT_LIVE): the stream (live) is null", N=7, k=2)
    sd = _lib.StreamDesc(S=64, H=32, L=8, n_streams=2, block=64, hop=16)
    live = dict(N=7, k=2, basis=p, moment=p, centre=p, lam=0.5, weight=p, state=p, ws=p, ws_bytes=1 << 24, live=C.pointer(sd))
    for change, text in ((dict(k=9), "L=8 outside [k=9, 512]"), (dict(weight=None), "weight (the amount of every stream) is null"),
                         (dict(state=None), "state (the diagnostics) is null"), (dict(lam=0.0), "lam=0 (epsilon)"),
                         (dict(ws_bytes=8), "ws_bytes=8, T=8 rows against N=7 columns")):
        _err(_lib.OT_LIVE, "rv_mosaic(OT_LIVE): " + text, **dict(live, **change))
    d = _lib.mosaic_call(_lib.OT_WORKSPACE, N=7, k=2, live=C.pointer(sd))
    assert d.ws_bytes == 256 + _lib.mosaic_call(_lib.OT_WORKSPACE, T=8, N=7, k=2).ws_bytes     # q [8, 8] fp32, then the map's


def test_the_wrappers_refuse_before_any_device_call():
    from rawaudiovae_kelsey_amd import transport as TR
    x32, y64 = torch.zeros(5, 4), torch.zeros(5, 2, dtype=torch.float64)
    for call in (lambda: TR.whiten(x32, torch.zeros(4, dtype=torch.float64), torch.zeros(2, 4, dtype=torch.float64)),
                 lambda: TR.whiten(None, None, None), lambda: TR.softmin(y64, y64, torch.zeros(10, dtype=torch.float64), 0.5),
                 lambda: TR.softmin(torch.zeros(5, 65, dtype=torch.float64), y64, y64, 0.5),
                 lambda: TR.transport_map(x32, y64, y64, y64, 0.5, 2), lambda: TR.workspace(0, 1, 1, "cpu"),
                 lambda: TR.workspace(1, 1, 65, "cpu"), lambda: TR.workspace(1, 1 << 31, 1, "cpu")):
        with pytest.raises(ValueError):
            call()
    for bad in (0, -1.0, float("inf"), float("nan"), 1e-60, 1e60, "x", None, True):
        with pytest.raises(ValueError, match="finite positive"):
            TR._epsilon(bad)
    assert TR._epsilon(0.1) == float(np.float32(0.1)) != 0.1
    with pytest.raises(TypeError, match="amount must be a number"):
        TR._amount("1", 1, "cpu")
    with pytest.raises(ValueError, match="amount=nan must be finite"):
        TR._amount(float("nan"), 1, "cpu")
    with pytest.raises(ValueError, match=r"float32 device tensor \[3\]"):
        TR._amount(torch.zeros(3), 3, "cpu")
    for kw, text in ((dict(n_components=0), "n_components=0"), (dict(n_components=65), "n_components=65"),
                     (dict(n_components=True), "n_components=True"), (dict(n_components=4, epsilon=0), "epsilon=0"),
                     (dict(n_components=4, epsilon="a"), "epsilon='a'"), (dict(n_components=4, tol=-1), "tol=-1"),
                     (dict(n_components=4, iters=0), "iters=0"), (dict(n_components=4, check_every=0), "check_every=0"),
                     (dict(n_components=4, level_iters=-1), "level_iters=-1"), (dict(n_components=4, level_iters=1.5), "level_iters=1.5")):
        with pytest.raises(ValueError, match=re.escape(text)):
            TR.LatentTransport(**kw)
    tr = TR.LatentTransport(4)
    with pytest.raises(RuntimeError, match="has not been fitted"):
        tr.map(x32)
    with pytest.raises(ValueError, match="x must be a 2-D float32 device tensor"):
        tr.fit(x32, x32)
    with pytest.raises(ValueError, match="no frame of the cloud is observed"):
        TR.log_weights(np.zeros(4, np.int32))
    levels, target = TR.schedule(0.05, 32.0, 10)
    assert target == float(np.float32(1.6)) and [e for e, _ in levels] == [32.0, 16.0, 8.0, 4.0, 2.0] and {n for _, n in levels} == {10}
    assert (levels, target) == O.schedule(0.05, 32.0, 10)
    assert TR.schedule(2.0, 32.0, 10) == ([], 64.0)


# ---- the file ---------------------------------------------------------------------------------------------------------------

def _host_transport(k=2, L=4, Ns=5, Nt=7):
    from rawaudiovae_kelsey_amd import transport as TR
    import states_oracle as SO
    rng = np.random.default_rng(3)
    c, P = SO.basis(k, L)
    t = lambda a: torch.from_numpy(np.array(a, dtype=np.float64))   # noqa: E731  (a copy: the oracle's arrays are read-only)
    lws = np.full(Ns, -np.log(Ns - 1.0))
    lws[2] = -np.inf
    tr = TR.LatentTransport(k, 0.07, iters=33)._set(
        t(c), t(P), t(O.unwhitening(P)), t(rng.standard_normal((Ns, k))), t(rng.standard_normal((Nt, k))),
        t(rng.standard_normal(Ns)), t(rng.standard_normal(Nt)), t(lws), t(np.full(Nt, -np.log(Nt))), 0.25, 41, 3e-4,
        [(30, 0.5), (40, 3e-4)], 1.75, 3.5)
    return tr


def test_the_file_round_trip_and_its_refusals(tmp_path):
    from rawaudiovae_kelsey_amd import transport as TR
    from rawaudiovae_kelsey_amd.frontend import check_fitted
    tr = _host_transport()
    path = str(tmp_path / "transport.npz")
    TR.write_transport(path, tr, 64, 16)
    back, meta = TR.read_transport(path, "cpu")
    assert meta == dict(segment_length=64, latent_dim=4, hop=16, n_source=5, n_target=7, n_iter=41)
    for name in ("mean_", "P_", "W_", "ys_", "yt_", "f_", "g_", "lws_", "lwt_"):
        a, b = getattr(tr, name).numpy(), getattr(back, name).numpy()
        assert a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64)), name
    assert (back.n_components, back.epsilon, back.epsilon_, back.n_iter_, back.err_, back.cost_, back.mean_cost_) == (
        2, 0.07, 0.25, 41, 3e-4, 1.75, 3.5)
    assert back.err_history_ == [(30, 0.5), (40, 3e-4)] and np.isneginf(back.lws_.numpy()[2])
    cfg = dict(segment_length=64, latent_dim=4)
    assert check_fitted("transport", path, meta, cfg, 16, "the transport was", "x") == 16
    with pytest.raises(ValueError, match="fitted for segment_length 64 and latent_dim 4, the model has 128 and 4"):
        check_fitted("transport", path, meta, dict(cfg, segment_length=128), 16)
    with pytest.raises(ValueError, match="fitted for segment_length 64 and latent_dim 4, the model has 64 and 8"):
        check_fitted("transport", path, meta, dict(cfg, latent_dim=8), 16)
    with pytest.raises(ValueError, match="--hop: hop 32: the transport was fitted at hop 16"):
        check_fitted("transport", path, meta, cfg, 32, "the transport was", "x")
    TR.write_transport(path, tr, 64, None)
    assert TR.read_transport(path, "cpu")[1]["hop"] is None
    with np.load(path) as z:
        parts = {n: z[n] for n in z.files}
    np.savez(path, **{n: v for n, v in parts.items() if n != "target_potential"})
    with pytest.raises(ValueError, match="not a latent-transport file, it lacks target_potential"):
        TR.read_transport(path, "cpu")
    np.savez(path, **dict(parts, source_potential=np.zeros(6)))
    with pytest.raises(ValueError, match=r"source_potential \(6,\) do not fit 2 components, latent_dim 4 and 5 \+ 7 frames"):
        TR.read_transport(path, "cpu")
    with pytest.raises(RuntimeError, match="has not been fitted"):
        TR.write_transport(path, TR.LatentTransport(2), 64)


def test_flag_parsing():
    import transfer as FE
    base = ["--checkpoint", "c"]
    a = FE.parse_args(["fit"] + base + ["--source", "s", "--target", "t", "--out", "o.npz"])
    assert (a.keep, a.epsilon, a.iters, a.tol, a.max_frames, a.hop, a.pca) == (16, 0.05, 500, 1e-3, 65536, None, None)
    a = FE.parse_args(["fit"] + base + ["--source", "s", "--target", "t", "--out", "o", "--keep", "4", "--hop", "16",
                                        "--epsilon", "0.5", "--iters", "7", "--tol", "0", "--max-frames", "100", "--pca", "p"])
    assert (a.keep, a.epsilon, a.iters, a.tol, a.max_frames, a.hop, a.pca) == (4, 0.5, 7, 0.0, 100, 16, "p")
    b = FE.parse_args(["apply"] + base + ["--transport", "t", "--in", "i", "--out", "o"])
    assert (b.window, b.amount, b.reverse, b.live_block, b.wav) == (None, 1.0, False, None, "i")
    b = FE.parse_args(["apply"] + base + ["--transport", "t", "--in", "i", "--out", "o", "--window", "hann", "--amount",
                                          "-0.5", "--reverse", "--live-block", "256", "--hop", "256"])
    assert (b.window, b.amount, b.reverse, b.live_block, b.hop) == ("hann", -0.5, True, 256, 256)
    fit = ["fit"] + base + ["--source", "s", "--target", "t", "--out", "o"]
    app = ["apply"] + base + ["--transport", "t", "--in", "i", "--out", "o"]
    for argv, text in ((fit + ["--keep", "0"], "--keep '0': expected a positive integer"),
                       (fit + ["--keep", "65"], "--keep 65: at most 64"),
                       (fit + ["--epsilon", "0"], "--epsilon '0': expected a finite number > 0"),
                       (fit + ["--iters", "x"], "--iters 'x': expected a positive integer"),
                       (fit + ["--tol", "-1"], "--tol '-1': expected a finite number >= 0"),
                       (fit + ["--max-frames", "0"], "--max-frames '0': expected a positive integer"),
                       (fit + ["--hop", "0"], "--hop '0': expected a positive integer"),
                       (app + ["--window", "hamming"], "--window 'hamming': expected none or hann"),
                       (app + ["--amount", "inf"], "--amount 'inf': expected a finite number"),
                       (app + ["--live-block", "0"], "--live-block '0': expected an integer >= 1"),
                       ([], "expected a command: fit or apply")):
        with pytest.raises(ValueError, match=re.escape(text)):
            FE.parse_args(argv)
    assert [FE.thin(T, 100) for T in (1, 100, 101, 200, 201)] == [1, 1, 2, 2, 3]
    assert len(range(0, 201, FE.thin(201, 100))) <= 100


# ---- the oracle against itself ----------------------------------------------------------------------------------------------

def _planted(n=40, k=3, seed=5):
    """The target cloud, and a source that is a permuted copy of it plus a constant shift"""
    rng = np.random.default_rng(seed)
    yt = rng.standard_normal((n, k)) * 2.0
    perm = rng.permutation(n)
    ys = yt[perm] + np.array([3.0, -1.0, 0.5])[:k]
    return ys, yt, perm


def test_row_marginals_hold_after_an_f_update_and_the_error_never_rises():
    ys, yt, _ = _planted()
    lws, lwt = O.log_weights(np.ones(40)), O.log_weights(np.ones(40))
    lwt[7] = lws[11] = -np.inf
    lws[lws > -np.inf] = lwt[lwt > -np.inf] = -np.log(39.0)
    eps = O.eps32(0.05 * O.mean_cost(ys[lws > -np.inf], yt[lwt > -np.inf]))
    g = np.random.default_rng(1).standard_normal(40)
    f = O.softmin(ys, yt, g, lwt, eps)
    Pm = O.plan(ys, lws, yt, lwt, f, g, eps)
    rows = Pm.sum(axis=1).astype(np.float64)
    assert np.abs(rows - np.exp(lws)).max() <= 1e-12 and rows[11] == 0 and (Pm[:, 7] == 0).all()
    res = O.sinkhorn(ys, lws, yt, lwt, 0.05, iters=200, tol=1e-9, level_iters=5, check_every=1)
    errs = [e for _, e in res["history"]]
    print("errors at the target epsilon:", errs[0], "->", errs[-1], "in", len(errs))
    assert len(errs) == 200 and all(b <= a * (1 + 1e-9) + 1e-15 for a, b in zip(errs, errs[1:])) and errs[-1] < 0.01 * errs[0]
    # ... the g-update that ended the loop holds the column marginals; the rows are off by what the next f-update will move
    Pm = O.plan(ys, lws, yt, lwt, res["f"], res["g"], res["epsilon"])
    assert np.abs(Pm.sum(axis=0).astype(np.float64) - np.exp(lwt)).max() <= 1e-12
    assert np.abs(Pm.sum(axis=1).astype(np.float64) - np.exp(lws)).sum() <= 2 * errs[-1]


def test_a_permuted_shifted_copy_is_mapped_onto_its_partners_and_back_as_epsilon_falls():
    ys, yt, perm = _planted()
    lw = O.log_weights(np.ones(40))
    worst = []
    for rel in (0.5, 0.05, 0.005):
        res = O.sinkhorn(ys, lw, yt, lw, rel, iters=3000, tol=1e-10, level_iters=10, check_every=10)
        there = O.transport_map(ys, yt, res["g"], lw, res["epsilon"])
        back = O.transport_map(there["T"], ys, res["f"], lw, res["epsilon"])
        worst.append((np.abs(there["T"] - yt[perm]).max(), np.abs(back["T"] - ys).max(), np.median(there["support"])))
    print("max |T(ys) - partner|, max |reverse(T(ys)) - ys|, median support per epsilon:", worst)
    assert worst[0][0] > worst[1][0] > worst[2][0] and worst[0][1] > worst[1][1] > worst[2][1]
    assert worst[0][2] > worst[1][2] > worst[2][2] and worst[2][2] < 1.01
    # at the smallest epsilon every row's image is nearer to its partner than to any other target point, and the reverse
    # map of the image nearer to the row it came from than to any other source point
    assert np.array_equal(O.costs(there["T"], yt).argmin(axis=1), perm)
    assert np.array_equal(O.costs(back["T"], ys).argmin(axis=1), np.arange(40))
    # the transport cost of the planted pair is the squared length of the shift
    assert abs(float((np.exp(lw) * there["cbar"]).sum()) - (9.0 + 1.0 + 0.25)) < 0.05


def test_the_exact_limit_case_has_its_gap():
    for k, N, T in ((1, 17, 33), (3, 515, 130), (64, 300, 65)):
        Q, V, near = O.lattice_case(k, N, T)
        assert np.abs(Q - V[near]).max() <= 0.25 and np.array_equal(V, np.round(V))
        c = O.costs(Q, V).astype(np.float64)
        first = c[np.arange(T), near]
        c[np.arange(T), near] = np.inf
        assert (c.min(axis=1) - first >= 0.5).all() and (first == c.min(axis=1).clip(max=0) + first).all()
        got = O.transport_map(Q, V, np.zeros(N), O.log_weights(np.ones(N)), 2.0 ** -11)
        assert np.array_equal(got["T"], V[near]) and (got["support"] == 1.0).all()
        assert np.exp(-0.5 * 2.0 ** 11) == 0.0


def test_the_oracle_tells_a_wrong_rule_from_the_right_one():
    A, B, h, cost = O.case(3, 15, 15)
    lw = O.log_weights(np.ones(15))
    eps = O.eps32(cost)
    f = O.softmin(A, B, h, lw, eps)
    ds, _ = O.delta_s(A, B, eps, 3)
    assert (np.abs(O.softmin(A, B, h, lw, O.eps32(cost * (1 + 1e-6))) - f) / eps > ds).any()    # another epsilon
    assert (np.abs(O.softmin(A, B, np.roll(h, 1), lw, eps) - f) / eps > ds).any()               # the potentials shifted
    lw2 = lw.copy()
    lw2[0] = -np.inf
    assert (np.abs(O.softmin(A, B, h, lw2, eps) - f) / eps > ds).any()                          # a column's weight ignored
    assert np.isposinf(O.softmin(A, B, h, np.full(15, -np.inf), eps)).all()
    far = O.softmin(A[:1], B, h, lw, O.eps32(0.01 * cost))
    assert np.isfinite(far).all() and far[0] > 1e5        # the row 10^3 standard deviations out: no overflow
