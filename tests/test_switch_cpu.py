"""The switching walk without a GPU: the op codes, descriptor roles and workspace sizes against the header, every argument
check of the five ops (they run before anything is launched), the .npz round trip and its refusals, compose.py's --form, and
the oracle against itself (tests/switch_oracle.py): the closure A A^T + B B^T = I of every state, the contraction guard at a
planted ||A||_2 = 1.5, the recovery of planted per-state dynamics, and that each restated sum tells a wrong rule from the
right one."""
import ctypes as C
import re
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from conftest import REPO  # noqa: E402
import abi_slots  # noqa: E402
import states_oracle as SO  # noqa: E402
import switch_oracle as O  # noqa: E402

sys.path.insert(0, REPO)


def test_op_codes_roles_and_workspace_sizes():
    from rawaudiovae_kelsey_amd import _lib
    text = open(REPO + "/include/rawvae_hip.h").read()
    codes = dict(re.findall(r"#define (RV_SWITCH_\w+) (\d+)", text))
    assert codes == dict(RV_SWITCH_RESIDUAL="52", RV_SWITCH_MOMENTS="53", RV_SWITCH_FIT="54", RV_SWITCH_STEP="55",
                         RV_SWITCH_WORKSPACE="56", RV_SWITCH_DYNAMICS="0", RV_SWITCH_NOISE="1")
    assert (_lib.SWITCH_RESIDUAL, _lib.SWITCH_MOMENTS, _lib.SWITCH_FIT, _lib.SWITCH_STEP, _lib.SWITCH_WORKSPACE) == (52, 53, 54, 55, 56)
    assert (_lib.SWITCH_DYNAMICS, _lib.SWITCH_NOISE) == (0, 1)
    assert _lib.SWITCH_WORKSPACE in _lib._HOST_ONLY_OPS
    assert not {_lib.SWITCH_RESIDUAL, _lib.SWITCH_MOMENTS, _lib.SWITCH_FIT, _lib.SWITCH_STEP} & _lib._HOST_ONLY_OPS
    para = text[text.index("/* Switching walk"):text.index("#define RV_SWITCH_RESIDUAL")]
    types = {n: ctype for slot in abi_slots.header_slots() for n, ctype in slot}
    for field, ctype in (("moment", "const double*"), ("result", "double*"), ("state", "double*"), ("info", "int*"),
                         ("path", "int*"), ("idx", "int*"), ("primed", "int*"), ("next_of", "const int*"),
                         ("weight", "const float*"), ("eigenvalues", "double*"), ("centre", "double*"), ("basis", "double*"),
                         ("q", "const float*"), ("out", "float*"), ("S", "long"), ("k", "long"), ("L", "long"), ("T", "long"),
                         ("stride", "long"), ("n_rows", "long"), ("mode", "long"), ("ldo", "long"), ("ws_bytes", "long")):
        assert re.search(r"\b%s\b" % field, para), field
        assert hasattr(_lib.MosaicDesc, field) and types[field] == ctype, (field, types.get(field))
    assert len(abi_slots.check_layout()) == 37 and C.sizeof(_lib.MosaicDesc) == 37 * 8
    assert _lib.lib().rv_version() == 100 and "switch" not in " ".join(_lib.EXPORTED)
    for op in (38, 39, 42, 48, 57):     # still unassigned
        with pytest.raises(_lib.RvError, match="unknown op %d" % op):
            _lib.lib().rv_mosaic(op, C.byref(_lib.MosaicDesc()), None)
    up = lambda n: -(-n // 256) * 256   # noqa: E731
    for T, S, k in ((5000, 17, 33), (2, 1, 1), (4097, 64, 64), (4098, 3, 3)):
        d = _lib.mosaic_call(_lib.SWITCH_WORKSPACE, T=T, S=S, k=k)
        pairs = T - 1
        assert d.ws_bytes == up(pairs) + up(-(-pairs // 256) * S * 8) + -(-pairs // 4096) * (S + 2) * 64 * 64 * 8, (T, S, k)


def _err(op, text, **fields):
    from rawaudiovae_kelsey_amd import _lib
    with pytest.raises(_lib.RvError) as e:
        _lib.lib().rv_mosaic(op, C.byref(_lib.MosaicDesc(**fields)), None)
    assert text in str(e.value), str(e.value)


def test_every_op_names_the_offending_field_before_it_launches():
    from rawaudiovae_kelsey_amd import _lib
    p = 0x1000     # never dereferenced: every call here fails a check
    res = dict(T=10, S=3, k=2, L=4, stride=4, q=p, centre=p, basis=p, moment=p, state=p, result=p)
    mom = dict(T=10, S=3, k=2, n_rows=2, row_start=p, ws=p, ws_bytes=1 << 24, moment=p, state=p, result=p)
    dyn = dict(S=3, k=2, mode=_lib.SWITCH_DYNAMICS, moment=p, result=2 * p, info=p)
    noi = dict(S=3, k=2, mode=_lib.SWITCH_NOISE, basis=p, moment=p, eigenvalues=p, result=p)
    ops = (("SWITCH_RESIDUAL", _lib.SWITCH_RESIDUAL, res), ("SWITCH_MOMENTS", _lib.SWITCH_MOMENTS, mom),
           ("SWITCH_FIT", _lib.SWITCH_FIT, dyn), ("SWITCH_FIT", _lib.SWITCH_FIT, noi),
           ("SWITCH_WORKSPACE", _lib.SWITCH_WORKSPACE, dict(T=10, S=3, k=2)))
    for name, op, ok in ops:
        for change, text in ((dict(S=0), "S=0 (the states) outside [1, 64]"), (dict(S=65), "S=65 (the states) outside [1, 64]"),
                             (dict(k=0), "k=0 (the axes) outside [1, 64]"), (dict(k=65), "k=65 (the axes) outside [1, 64]")):
            _err(op, "rv_mosaic(%s): %s" % (name, text), **dict(ok, **change))
    _err(_lib.SWITCH_RESIDUAL, "T=0 outside [1, 2^31)", **dict(res, T=0))
    for name, op, ok in (ops[1], ops[4]):
        _err(op, "rv_mosaic(%s): T=1 outside [2, 2^31)" % name, **dict(ok, T=1))
        _err(op, "rv_mosaic(%s): T=2147483648 outside [2, 2^31)" % name, **dict(ok, T=1 << 31))
    for change, text in ((dict(L=1), "L=1 outside [k=2, 512]"), (dict(L=513, stride=513), "L=513 outside [k=2, 512]"),
                         (dict(stride=3), "stride=3 (the row pitch of x) holds no row of L=4 values"),
                         (dict(q=None), "q (the latent rows x) is null"), (dict(centre=None), "centre is null"),
                         (dict(basis=None), "basis (P) is null"), (dict(moment=None), "moment (theta) is null"),
                         (dict(state=None), "state (gamma) is null"), (dict(result=None), "result (the residual block) is null"),
                         (dict(result=p + 8), "result is not 256-byte aligned")):
        _err(_lib.SWITCH_RESIDUAL, "rv_mosaic(SWITCH_RESIDUAL): " + text, **dict(res, **change))
    for change, text in ((dict(n_rows=0), "n_rows=0 (the files) outside [1, 2^31)"), (dict(row_start=None), "row_start is null"),
                         (dict(moment=None), "moment (the residual block) is null"),
                         (dict(moment=p + 8), "moment is not 256-byte aligned"), (dict(state=None), "state (gamma) is null"),
                         (dict(result=None), "result (the moments) is null"),
                         (dict(ws_bytes=8), "ws_bytes=8, T=10 frames of S=3 states need"),
                         (dict(ws=None), "ws is null, T=10 frames"), (dict(ws=p + 8), "ws is not 256-byte aligned")):
        _err(_lib.SWITCH_MOMENTS, "rv_mosaic(SWITCH_MOMENTS): " + text, **dict(mom, **change))
    _err(_lib.SWITCH_FIT, "mode=2 is neither RV_SWITCH_DYNAMICS nor RV_SWITCH_NOISE", **dict(dyn, mode=2))
    for change, text in ((dict(moment=None), "moment (the moments) is null"), (dict(info=None), "info is null"),
                         (dict(result=None), "result is null"), (dict(result=p), "result and moment are the same block")):
        _err(_lib.SWITCH_FIT, "rv_mosaic(SWITCH_FIT): " + text, **dict(dyn, **change))
    for change, text in ((dict(basis=None), "basis (A) is null"), (dict(moment=None), "moment (the eigenvectors of Q) is null"),
                         (dict(eigenvalues=None), "the eigenvalues of Q are null"), (dict(result=None), "result is null")):
        _err(_lib.SWITCH_FIT, "rv_mosaic(SWITCH_FIT): " + text, **dict(noi, **change))
    _err(_lib.SWITCH_STEP, "rv_mosaic(SWITCH_STEP): the stream (live) is null", S=3, k=2, L=4)


# ---- the file ---------------------------------------------------------------------------------------------------------------

def _host_model(S=3, k=2, L=4):
    from rawaudiovae_kelsey_amd import states as ST
    from rawaudiovae_kelsey_amd import switching as SW
    c, P = SO.basis(k, L)
    th = SO.random_theta(S, k)
    st = ST.LatentStates(S, k, 2e-3)._set(torch.from_numpy(th), torch.from_numpy(c.copy()), torch.from_numpy(P.copy()), 77, 3)
    phi = torch.from_numpy(O.random_phi(S, k))
    R = torch.from_numpy(np.linalg.solve(P @ P.T, P))
    sw = SW.SwitchingWalk(st)._set(phi, st.mean_, st.P_, R, [5.0, 6.5, 0.0], [1.0, 0.8, 1.0], [0, 0, 1], 77, 3)
    return st, sw


def test_the_file_round_trip_and_its_refusals(tmp_path):
    from rawaudiovae_kelsey_amd import switching as SW
    st, sw = _host_model()
    path = str(tmp_path / "form.npz")
    SW.write_switching(path, sw, 64, 16)
    back, meta = SW.read_switching(path, "cpu")
    assert meta == dict(segment_length=64, latent_dim=4, hop=16, n_frames=77, n_files=3)
    for name in ("phi_", "mean_", "P_", "R_"):
        assert torch.equal(getattr(back, name), getattr(sw, name)), name
    assert torch.equal(back.states.theta_, st.theta_) and back.states.var_floor == 2e-3
    assert np.array_equal(back.pairs_, [5.0, 6.5, 0.0]) and np.array_equal(back.shrink_, [1.0, 0.8, 1.0])
    assert np.array_equal(back.info_, [0, 0, 1]) and (back.n_states, back.n_components) == (3, 2)
    a = back.dyn_[:, 0].numpy()
    assert np.allclose(back.predictability_, (a * a).sum(axis=(1, 2)) / 2) and back.dyn_.shape == (3, 2, 2, 2)
    assert np.allclose(back.R_.numpy() @ back.P_.numpy().T, np.eye(2), atol=1e-12)          # R un-whitens
    SW.write_switching(path, sw, 64)
    assert SW.read_switching(path, "cpu")[1]["hop"] is None
    # refusals: a states file is no switching file; arrays that do not fit one another
    from rawaudiovae_kelsey_amd import states as ST
    other = str(tmp_path / "states.npz")
    ST.write_states(other, st, 64, 16)
    with pytest.raises(ValueError, match="not a latent-switching file, it lacks phi, unwhiten"):
        SW.read_switching(other, "cpu")
    with np.load(path) as z:
        parts = {n: z[n] for n in z.files}
    for change in (dict(phi=parts["phi"][:-1]), dict(unwhiten=parts["unwhiten"][:, :3]), dict(n_states=np.int64(4)),
                   dict(pairs=parts["pairs"][:2]), dict(n_components=np.int64(65))):
        with open(path, "wb") as f:
            np.savez(f, **dict(parts, **change))
        with pytest.raises(ValueError, match="do not fit"):
            SW.read_switching(path, "cpu")
    with pytest.raises(TypeError, match="needs a fitted LatentStates"):
        SW.SwitchingWalk(sw)
    with pytest.raises(RuntimeError, match="has not been fitted"):
        SW.write_switching(path, SW.SwitchingWalk(st), 64)


# ---- --form ---------------------------------------------------------------------------------------------------------------

def test_form_parsing_and_its_messages():
    import compose as CP
    assert CP.parse_form("A:2,B:1.5,*:4,A:2") == [(0, 2.0), (1, 1.5), (CP.FREE, 4.0), (0, 2.0)]
    assert CP.parse_form(" Z:0.25 , 26:1") == [(25, 0.25), (26, 1.0)]
    for bad, msg in (("A", "expected LETTER:SECONDS"), ("A:x", "expected LETTER:SECONDS"), ("A:0", "duration must be"),
                     ("A:-1", "duration must be"), ("A:inf", "duration must be"), ("A:nan", "duration must be"),
                     ("a:1", "unknown letter 'a'"), ("AB:1", "unknown letter 'AB'"), ("3:1", "unknown letter '3'"),
                     (":1", "unknown letter ''"), ("A:1,,B:1", "expected LETTER:SECONDS")):
        with pytest.raises(ValueError, match="--form %s: .*%s" % (re.escape(repr(bad)), msg)):
            CP.parse_form(bad)
    with pytest.raises(ValueError, match="--form 'A:1,D:2': unknown letter D: the model has 3 states \\(A .. C\\)"):
        CP.check_form(CP.parse_form("A:1,D:2"), 3, "A:1,D:2")
    assert CP.check_form(CP.parse_form("C:1,*:2"), 3, "C:1,*:2")[0] == (2, 1.0)
    # seconds rounded to frames, the rest free, a form longer than the run cut
    f = CP.form_frames(CP.parse_form("A:0.5,*:0.25,B:0.26"), 12, 16, 2)            # 8 frames per second
    assert f.tolist() == [0, 0, 0, 0, -1, -1, 1, 1, -1, -1, -1, -1] and f.dtype == np.int32
    assert CP.form_frames(CP.parse_form("B:10"), 5, 16, 2).tolist() == [1] * 5
    assert CP.form_frames(CP.parse_form("B:0.01,A:1"), 3, 16, 2).tolist() == [1, 0, 0]          # at least one frame
    assert CP.form_frames([], 3, 16, 2).tolist() == [-1] * 3
    base = ["run", "--checkpoint", "c", "--model", "m", "--out", "o", "--seconds", "1"]
    args = CP.parse_args(base + ["--form", "A:1,*:2"])
    assert args.form == [(0, 1.0), (CP.FREE, 2.0)] and args.form_text == "A:1,*:2" and args.window is None
    assert CP.parse_args(base).form == []
    for flags, msg in ((["--form", "q:1"], "--form 'q:1': unknown letter 'q'"), (["--streams", "0"], "--streams '0'"),
                       (["--seed", "-1"], "--seed '-1'"), (["--temperature", "-1"], "--temperature '-1'"),
                       (["--window", "hamming"], "--window 'hamming'"), (["--hop", "0"], "--hop '0'")):
        with pytest.raises(ValueError, match=re.escape(msg)):
            CP.parse_args(base + flags)
    with pytest.raises(ValueError, match="--seconds '0'"):
        CP.parse_args(base[:-1] + ["0"])
    with pytest.raises(ValueError, match="expected a command"):
        CP.parse_args([])
    assert CP.out_paths("a/b.json", 1) == ["a/b.json"] and CP.out_paths("a/b.json", 2) == ["a/b_0.json", "a/b_1.json"]


# ---- the oracle's own invariants ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("S,k", SO.MSTEP_SHAPES)
def test_closure_of_every_state(S, k):
    x, c, P, th, gamma, rs = O.moments_case(S, k, 300, (100, 0, 200), (150,))
    f = O.fit(x, rs, c, P, th, gamma, S, k)
    worst = O.closure(f["dyn"])
    norms = [np.linalg.norm(d[0], 2) for d in f["dyn"]]
    print("S %d k %d: closure %.3g, ||A||_2 up to %.6f, g from %.4f, thin states %d" % (
        S, k, worst, max(norms), f["g"].min(), f["info"].sum()))
    assert worst <= 64 * k * O.U and max(norms) <= 1 + 1e-12
    assert np.array_equal(f["Q"], np.swapaxes(f["Q"], 1, 2))                    # bitwise symmetric
    thin = f["info"] == 1
    assert np.array_equal(thin, ~(f["mo"]["N"] >= 2)) and not f["A"][thin].any() and (f["g"][thin] == 1).all()
    assert (f["g"] <= 1).all() and (f["g"] > 0).all()
    assert f["obs"].sum() == 299 and not f["r"][150].any() and not f["keep"][[99, 149, 150]].any() and f["keep"].sum() == 296


def test_the_guard_at_a_planted_norm_of_one_and_a_half():
    k = 4
    rng = np.random.default_rng(2)
    a = rng.standard_normal((k, k))
    a *= 1.5 / np.linalg.norm(a, 2)
    D = rng.uniform(0.5, 2, k)
    mo = dict(N=np.array([100.0]), Dn=D[None], Dt=D[None], C1=(a * np.sqrt(D)[:, None] * np.sqrt(D)[None, :])[None])
    A, Q, info = O.dynamics(mo)
    assert np.allclose(A[0], a, rtol=1e-14) and info[0] == 0
    q, Uv = O.eigh_desc(Q)
    assert q.min() < 0 and np.isclose(q.min(), 1 - 1.5 ** 2)
    dyn, g = O.noise(A, Uv, q)
    print("guard: g %.17g (1 / 1.5 = %.17g), closure %.3g" % (g[0], 1 / 1.5, O.closure(dyn)))
    assert abs(g[0] - 1 / 1.5) <= 4 * O.U and abs(np.linalg.norm(dyn[0, 0], 2) - 1) <= 1e-14
    assert O.closure(dyn) <= 64 * k * O.U
    # a contraction is left alone: g = 1 and A bit for bit
    mo["C1"] = mo["C1"] / 3
    A, Q, _ = O.dynamics(mo)
    q, Uv = O.eigh_desc(Q)
    dyn, g = O.noise(A, Uv, q)
    assert g[0] == 1 and np.array_equal(dyn[0, 0], A[0].T) and O.closure(dyn) <= 64 * k * O.U


def test_planted_dynamics_are_recovered():
    x, rs, th, labels, At = O.planted()
    assert x.shape == (12000, 2) and rs.tolist() == [0, 3000, 6000, 9000, 12000]
    f = O.planted_fit()
    N = f["mo"]["N"]
    A = f["A"]
    err = np.abs(A - At).max(axis=(1, 2))
    print("planted: N %s, max |A_j - planted| %s, gate 8 / sqrt(N) %s, shrink %s" % (N, err, 8 / np.sqrt(N), f["g"]))
    assert (err <= 8 / np.sqrt(N)).all() and (N > 1000).all() and f["info"].sum() == 0
    assert abs(N.sum() - (12000 - 4)) < 1e-6                                   # every pair inside a file, once
    assert (f["g"] == 1).all() and O.closure(f["dyn"]) <= 64 * 2 * O.U


def test_each_restated_sum_tells_a_wrong_rule_from_the_right_one():
    S, k, T = 3, 3, 300
    x, c, P, th, gamma, rs = O.moments_case(S, k, T, (100, 200), (150,))
    r, obs = O.residual(x, c, P, th, gamma, S, k)
    keep = O.keep_mask(rs, obs, T)
    right = O.pack_moments(O.moments(r, gamma, keep))
    # a dropped file end: pair 99 spans the files
    no_end = O.keep_mask(rs, obs, T, file_ends=False)
    assert no_end[99] and not keep[99] and no_end.sum() == keep.sum() + 1
    wrong = O.pack_moments(O.moments(r, gamma, no_end))
    assert (wrong != right).sum() > right.size // 2
    # an ungated unobserved frame: r is +0 there, so C1, D' and D agree; N tells
    ungated = O.keep_mask(rs, obs, T, gate=False)
    assert ungated[149] and ungated[150] and not keep[149] and not keep[150]
    mo_u, mo_r = O.moments(r, gamma, ungated), O.moments(r, gamma, keep)
    assert (mo_u["N"] != mo_r["N"]).all() and (mo_u["Dn"] != mo_r["Dn"]).any()   # gamma'_151 r_151^2 enters D' through pair 150
    # gamma_p in place of gamma_{p+1}
    wrong = O.pack_moments(O.moments(r, gamma, keep, this_gamma=True))
    assert (wrong != right).sum() > right.size // 2
    # the residual: the chain over the states in descending order differs in the last bits somewhere
    p = SO.unpack(th, S, k)
    y = SO.whiten(x, c, P)
    rev = np.zeros_like(y)
    for i in reversed(range(S)):
        rev = SO.fma(gamma[:, i][:, None], (y - p["m"][i][None, :]) * np.sqrt(p["w"][i])[None, :], rev)
    rev[~obs.astype(bool)] = 0
    assert (rev != r).any() and np.allclose(rev, r, rtol=1e-12, atol=1e-12)
    # against plain numpy sums: the same numbers up to rounding
    g1 = gamma[1:] * keep[:, None]
    assert np.allclose(mo_r["N"], g1.sum(0), rtol=1e-12)
    assert np.allclose(mo_r["C1"], np.einsum("pj,pa,pb->jab", g1, r[1:], r[:-1]), rtol=0, atol=1e-10)
    assert np.allclose(mo_r["Dn"], g1.T @ (r[1:] ** 2), rtol=0, atol=1e-10)
    assert np.allclose(mo_r["Dt"], g1.T @ (r[:-1] ** 2), rtol=0, atol=1e-10)


def test_the_step_oracle_draws_states_by_the_header():
    assert O.draw_state([0.25, 0.25, 0.5], np.float32(0.25)) == 1              # on an edge: the next state
    assert O.draw_state([0.25, 0.25, 0.5], np.float32(0.2499)) == 0
    assert O.draw_state([0.5, 0.0, 0.5, 0.0], np.float32(0.5)) == 2            # a zero-probability state is never drawn
    assert O.draw_state([0.5, 0.25, 0.0], np.float32(0.99999994)) == 1          # none qualifies: the highest positive one
    assert O.draw_state([0.0, 0.0], np.float32(0.3)) == 0
    u = [O.state_uniform(7, f, s) for f in range(3) for s in range(2)]
    assert len(set(float(v) for v in u)) == 6 and all(0 < v < 1 and v.dtype == np.float32 for v in u)
    # forced states are taken as given; the state sequence is continuous: a forced frame moves the same u on
    S, k, L = 3, 2, 4
    phi = O.random_phi(S, k)
    c, P = SO.basis(k, L)
    R = np.linalg.solve(P @ P.T, P)
    rng = np.random.default_rng(0)
    eps = rng.standard_normal((6, k)).astype(np.float32)
    un = rng.uniform(size=6).astype(np.float32)
    u1, cur, path, z = O.step(phi, R, c, S, k, np.zeros(k), False, 0, eps, un, [2, -1, -1, 1, 7, -1])
    assert path[0] == 2 and path[3] == 1 and cur == path[-1] and z.dtype == np.float32 and np.isfinite(z).all()
    ua, ca, pa, za = O.step(phi, R, c, S, k, np.zeros(k), False, 0, eps[:3], un[:3], [2, -1, -1])
    ub, cb, pb, zb = O.step(phi, R, c, S, k, ua, True, ca, eps[3:], un[3:], [1, 7, -1])
    assert np.array_equal(np.concatenate([pa, pb]), path) and np.array_equal(np.concatenate([za, zb]), z)
    assert np.array_equal(ub, u1)
