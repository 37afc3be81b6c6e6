"""Live mosaicing with a lag on the GPU (k_live_lag / RV_MOSAIC_LIVE_DRAIN in csrc/mosaic_live.hip,
StreamingMosaic(lag=D), drain(), mosaic.py --lag).  The committed choices are checked bit for bit against
tests/live_lag_oracle.py on the device's own candidates, the audio against the oracle's block player, lag 0
against the default construction."""
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from conftest import REPO  # noqa: E402
import live_lag_oracle as G  # noqa: E402
import live_mosaic_oracle as LO  # noqa: E402
import mosaic_oracle as O  # noqa: E402
import mosaic_path_oracle as P  # noqa: E402


def _M():
    from rawaudiovae_kelsey_amd import mosaic
    return mosaic


def _model(S=64, H=96, L=8, seed=0):
    from rawvae.model import VAE
    torch.manual_seed(seed)
    return VAE(S, H, L).cuda().eval()


def _waves(rng, lengths, sr=8000.0):
    out = []
    for i, n in enumerate(lengths):
        t = np.arange(n) / sr
        w = 0.6 * np.sin(2 * np.pi * (150 + 170 * i) * t) + 0.2 * rng.standard_normal(n)
        w[: n // 5] = 0                                          # leading silence: duplicate all-zero frames
        out.append(w.astype(np.float32))
    return out


def _index(model, hop, lengths=(700, 1000, 513, 1290), seed=9):
    index = _M().LatentIndex(model, hop=hop)
    for i, w in enumerate(_waves(np.random.default_rng(seed), lengths)):
        index.add(w, "f%d" % i)
    return index


def _signal(rng, n_streams, n):
    t = np.arange(n)
    x = np.stack([0.5 * np.sin(t * (0.05 + 0.03 * s)) for s in range(n_streams)]) + 0.1 * rng.standard_normal(
        (n_streams, n))
    return torch.from_numpy(x.astype(np.float32)).cuda()


def _run(sm, x, calls=None, replay=False, before_call=None):
    """`calls`: a string of 'p' (the next block of x through process) and 'd' (drain); None: every block of x, then
    sm.drain_blocks drains (none at lag 0) -> (y [n_streams, len(calls) * block], idx [n_streams, T, k], dist (of
    the frames fed), choice [n_streams, len(calls) * F] (as emitted, call after call), calls)."""
    if calls is None:
        calls = "p" * (x.shape[1] // sm.block) + "d" * (sm.drain_blocks if sm.lag else 0)
    ys, idxs, dists, choices = [], [], [], []
    b = 0
    for n, c in enumerate(calls):
        if before_call is not None:
            before_call(n)
        if c == "p":
            xb = x[:, b * sm.block:(b + 1) * sm.block]
            b += 1
            ys.append((sm.replay(xb) if replay else sm.process(xb)).clone())
            i, d, ch = sm.last_matches()
            idxs.append(i.clone()), dists.append(d.clone())
        else:
            ys.append((sm.drain_replay() if replay else sm.drain()).clone())
            ch = sm.last_matches()[2]
        choices.append(ch.clone())
    return torch.cat(ys, 1), torch.cat(idxs, 1), torch.cat(dists, 1), torch.cat(choices, 1), calls


def _expected(index, sm, idx_s, dist_s, calls, weight_of_call, adv=1):
    """The oracle's emitted choices of one stream for the device's own candidates -> (want [len(calls) * F], emit, choice)."""
    fb = sm.frames_per_block
    last, emit, T = G.schedule(calls, fb, sm.lag)
    assert T == idx_s.shape[0]
    w = np.zeros(T)
    for pos, a in enumerate(emit):
        if a >= 0:
            w[a] = weight_of_call(pos // fb)
    _, choice, _ = G.fixed_lag(idx_s, dist_s, index.mu.cpu().numpy(), index.successor(adv), w, sm.lag, last=last)
    return np.where(emit >= 0, choice[np.maximum(emit, 0)], -1), emit, choice


def _decoded(index, rows):
    """[len(rows), S] fp32: corpus rows (-1: the zero latent) through the offline decoder, as LatentIndex.mosaic decodes"""
    M = _M()
    from rawaudiovae_kelsey_amd._lib import ACT_RELU, ACT_TANH, ptr
    i = torch.from_numpy(np.asarray(rows, np.int32)).cuda().view(-1, 1)
    n = i.shape[0]
    z = M.gather_mean(index.mu, i, index.L, stride=index.L, n_rows=len(index))
    h = torch.empty((n, index.H), dtype=torch.float32, device="cuda")
    out = torch.empty((n, index.S), dtype=torch.float32, device="cuda")
    index.codec.linear(ptr(z), index.L, n, "fc3", ACT_RELU, ptr(h), index.H)
    index.codec.linear(ptr(h), index.H, n, "fc4", ACT_TANH, ptr(out), index.S)
    return out.cpu().numpy()


def _played(index, sm, emit, choice, mode, window):
    from rawaudiovae_kelsey_amd.stream import window_values
    w = None if window is None else window_values(sm.S, window)
    if mode == "grains":
        audio = index.audio.cpu().numpy()
        return G.play(emit, choice, lambda i: O.gather_mean(audio, index.row_start, np.array([[i]]), sm.S)[0], sm.S, sm.hop, w)
    table = _decoded(index, np.concatenate([[-1], choice]))
    return G.play(emit, np.arange(len(choice)), lambda a: table[1 + a], sm.S, sm.hop, w, blank=table[0])


def _eq(a, b):
    """bit for bit: floats are compared as int32 views"""
    if a.dtype == torch.float32:
        return b.dtype == torch.float32 and torch.equal(a.view(torch.int32), b.view(torch.int32))
    return torch.equal(a, b)


def test_lag_zero_given_explicitly_is_the_default_construction():
    M = _M()
    index = _index(_model(seed=2), 16)
    x = _signal(np.random.default_rng(1), 2, 32 * 6)
    for mode, cont in (("grains", 0.5), ("decode", 0.5), ("grains", 0.0)):
        kw = dict(hop=16, k=4, mode=mode, window="hann", continuity=cont)
        a, b = M.StreamingMosaic(index, 2, 32, **kw), M.StreamingMosaic(index, 2, 32, lag=0, **kw)
        assert b.lag == 0 and b.lag_samples == 0 and a._ws.numel() == b._ws.numel()
        assert all(_eq(p, q) for p, q in zip(_run(a, x)[:4], _run(b, x)[:4]))
        with pytest.raises(ValueError, match="lag"):
            b.drain()
    with pytest.raises(ValueError, match="lag"):
        M.StreamingMosaic(index, 2, 32, hop=16, k=4, continuity=0.0, lag=2)
    with pytest.raises(ValueError, match="lag"):
        M.StreamingMosaic(index, 2, 32, hop=16, k=4, continuity=0.5, lag=65)


@pytest.mark.parametrize("lag,mode,window", [(1, "grains", "hann"), (3, "grains", "hann"), (8, "grains", "hann"),
                                             (64, "grains", "hann"), (3, "grains", None), (3, "decode", "hann"),
                                             (8, "decode", None)])
def test_choices_follow_the_oracle_across_blocks_and_the_audio_its_player(lag, mode, window):
    M = _M()
    S, hop, block, k = 64, 16, 32, 8
    index = _index(_model(seed=5), hop)
    sm = M.StreamingMosaic(index, 2, block, hop=hop, k=k, mode=mode, window=window, continuity=0.5, lag=lag)
    assert sm.lag == lag and sm.lag_samples == lag * hop and sm.latency == S - hop
    n_blocks = 10
    x = _signal(np.random.default_rng(4), 2, n_blocks * block)
    weights = {b: (0.5, 0.5) for b in range(n_blocks)}
    for b in range(4, n_blocks):
        weights[b] = (3.0, 0.0)                                  # a weight change between blocks
    weights[8] = (float("nan"), -2.0)                            # not finite and >= 0: counts as 0

    def weight_at(call):                                         # the drains run under the last block's weights
        return weights[min(call, n_blocks - 1)]

    def before(call):
        sm.weight.copy_(torch.tensor(weight_at(call), device="cuda"))
        # block 6 of stream 1 has no candidates: a NaN query row matches nothing
        sm.offset[1, 0] = float("nan") if call == 6 else 0.0

    y, idx, dist, choice, calls = _run(sm, x, before_call=before)
    assert calls == "p" * n_blocks + "d" * -(-(lag + 3) // 2)
    y, idx, dist, choice = [t.cpu().numpy() for t in (y, idx, dist, choice)]
    fb = block // hop
    assert np.all(idx[1, 6 * fb:7 * fb] == -1)
    assert np.all(choice[:, :min(lag, n_blocks * fb)] == -1)     # the warm-up: nothing is committed before a drain
    moved = 0
    for s in range(2):
        want, emit, committed = _expected(index, sm, idx[s], dist[s], calls, lambda c: weight_at(c)[s])
        assert np.array_equal(choice[s], want), np.argwhere(choice[s] != want)[:5]
        assert np.array_equal(np.sort(emit[emit >= 0]), np.arange(n_blocks * fb))   # every frame fed was committed
        moved += int(((idx[s] == committed[:, None]).argmax(1)[committed >= 0] > 0).sum())
        ref = _played(index, sm, emit, committed, mode, window)
        bad = np.argwhere(y[s].view(np.int32) != ref.view(np.int32))
        assert bad.size == 0, (s, bad[:5].ravel().tolist(), float(np.abs(y[s] - ref).max()))
    assert moved > 0                                             # the weight did change choices
    assert np.abs(y).max() > 0


def test_block_size_invariance_with_a_lag():
    M = _M()
    index = _index(_model(seed=3), 16)
    x = _signal(np.random.default_rng(2), 1, 16 * 8 * 4)
    for mode, lag in (("grains", 3), ("decode", 8)):
        outs = []
        for block in (16, 32, 128):
            sm = M.StreamingMosaic(index, 1, block, hop=16, k=4, mode=mode, window="hann", continuity=0.3, lag=lag)
            y, idx, dist, choice, _ = _run(sm, x)
            outs.append((y, idx, dist, choice))
        n = x.shape[1] + (lag + 3) * 16                          # everything fed has been played by then
        f = n // 16
        for o in outs:
            assert o[0].shape[1] >= n
        for o in outs[1:]:
            assert _eq(o[0][:, :n], outs[0][0][:, :n]) and _eq(o[1], outs[0][1]) and _eq(o[2], outs[0][2])
            assert torch.equal(o[3][:, :f], outs[0][3][:, :f])
        assert torch.all(outs[0][3][:, lag:lag + x.shape[1] // 16] >= 0)


def test_streams_are_independent_and_reset_restarts_one_with_its_pending_rows():
    M = _M()
    index = _index(_model(seed=4), 16)
    kw = dict(hop=16, k=4, mode="grains", window="hann", continuity=0.4, lag=5)
    x = _signal(np.random.default_rng(3), 3, 32 * 6)
    sm3 = M.StreamingMosaic(index, 3, 32, **kw)
    got = _run(sm3, x)[:4]
    for s in range(3):
        one = _run(M.StreamingMosaic(index, 1, 32, **kw), x[s:s + 1])[:4]
        assert all(_eq(a[s:s + 1], b) for a, b in zip(got, one)), s
    # reset(1) after three blocks: stream 1 starts over, its five pending rows forgotten; streams 0 and 2 carry on
    calls = "pppppp" + "d" * sm3.drain_blocks
    sm3 = M.StreamingMosaic(index, 3, 32, **kw)
    first = _run(sm3, x[:, :96], calls="ppp")[:4]
    sm3.reset(1)
    second = _run(sm3, x[:, 96:], calls=calls[3:])[:4]
    for s in (0, 2):
        assert all(_eq(torch.cat([a[s], b[s]]), g[s]) for a, b, g in zip(first, second, got))
    fresh = _run(M.StreamingMosaic(index, 1, 32, **kw), x[1:2, 96:], calls=calls[3:])[:4]
    assert all(_eq(a[1:2], b) for a, b in zip(second, fresh))
    assert torch.all(second[3][1, :5] == -1) and torch.all(second[3][0, :5] >= 0)
    sm3.reset()
    again = _run(sm3, x)[:4]
    assert all(_eq(a, b) for a, b in zip(again, got))


def test_more_rows_than_the_few_query_search_serves_give_the_same_bits_with_a_lag():
    M = _M()
    index = _index(_model(seed=7), 16)
    kw = dict(hop=16, k=4, mode="grains", window="hann", continuity=0.6, lag=4)
    x = _signal(np.random.default_rng(6), 5, 256 * 3)
    wide = M.StreamingMosaic(index, 5, 256, **kw)                # 80 rows per block: the tile search
    narrow = M.StreamingMosaic(index, 5, 32, **kw)               # 10 rows: the few-query search
    assert wide.n_streams * wide.frames_per_block > M.SMALL_T_MAX >= narrow.n_streams * narrow.frames_per_block
    a, b = _run(wide, x, calls="pppd"), _run(narrow, x, calls="p" * 24 + "d" * 8)
    assert all(_eq(p, q) for p, q in zip(a[:4], b[:4]))
    assert torch.all(a[3][:, 4:48 + 4] >= 0)


def test_graph_replay_equals_eager_sees_weight_edits_and_drains_between_blocks():
    from rawaudiovae_kelsey_amd._lib import RvError
    M = _M()
    index = _index(_model(seed=6), 16)
    kw = dict(hop=16, k=4, mode="decode", window="hann", continuity=0.5, lag=3)
    x = _signal(np.random.default_rng(5), 2, 32 * 8)
    eager, graph = M.StreamingMosaic(index, 2, 32, **kw), M.StreamingMosaic(index, 2, 32, **kw)
    with pytest.raises(RvError):
        graph.drain_replay()
    graph.capture()
    graph.reset()
    calls = "pppdppddpppddd"                                     # a partial drain, a dry one, then the full one

    def edit(sm):
        def before(call):
            if call == 5:
                sm.weight.fill_(4.0)
        return before

    a = _run(eager, x, calls=calls, before_call=edit(eager))
    b = _run(graph, x, calls=calls, replay=True, before_call=edit(graph))
    assert all(_eq(p, q) for p, q in zip(a[:4], b[:4]))
    y, idx, dist, choice = [t.cpu().numpy() for t in b[:4]]
    changed = 0
    for s in range(2):
        want, emit, committed = _expected(index, graph, idx[s], dist[s], calls, lambda c: 0.5 if c < 5 else 4.0)
        assert np.array_equal(choice[s], want), np.argwhere(choice[s] != want)[:5]
        flat, _, _ = _expected(index, graph, idx[s], dist[s], calls, lambda c: 0.5)
        changed += int((flat != want).sum())
        ref = _played(index, graph, emit, committed, "decode", "hann")
        assert np.array_equal(y[s].view(np.int32), ref.view(np.int32))
    assert changed > 0                                           # the replayed graph read the edited weight
    assert (G.schedule(calls, 2, 3)[1] == -1).sum() > 3          # the dry drain did emit empty frames after the warm-up


def _two_file_index(model, mu, F):
    """An index of two files of F frames whose corpus latents are replaced by mosaic_path_oracle.two_file_case's mu"""
    S = model.fc1.in_features
    index = _M().LatentIndex(model, hop=None)
    rng = np.random.default_rng(0)
    for i in range(2):
        index.add((0.3 * rng.standard_normal(F * S)).astype(np.float32), "file%d" % i)
    assert len(index) == 2 * F
    index._tables()["mu"] = torch.from_numpy(mu).cuda()
    return index


@pytest.mark.parametrize("lag", [0, 1, 64])
def test_two_file_case_on_the_device(lag):
    """One frame per block, scale = 0 and offset = q_t: the query is exactly q_t.  Lag 0 walks the greedy path
    (J = 12.9375, a file switch at every frame); one frame of look-ahead, or 64, finds best_path's (J = 10.5625)."""
    M = _M()
    F, L, w = 40, 8, 3 / 16
    mu, q, next_of = P.two_file_case(F, L, 0)
    model = _model(seed=8)
    index = _two_file_index(model, mu, F)
    assert np.array_equal(index.successor(1), next_of)
    sm = M.StreamingMosaic(index, 1, 64, k=2, mode="grains", continuity=w, lag=lag)
    assert sm.frames_per_block == 1
    sm.scale.zero_()
    qd = torch.from_numpy(q).cuda()

    def before(call):
        if call < F:
            sm.offset[0].copy_(qd[call])

    x = _signal(np.random.default_rng(7), 1, F * 64)
    y, idx, dist, choice, calls = _run(sm, x, before_call=before)
    idx, dist, choice = idx[0].cpu().numpy(), dist[0].cpu().numpy(), choice[0].cpu().numpy()
    ri, rd = O.knn(q, mu, 2)
    assert np.array_equal(idx, ri) and np.array_equal(dist.view(np.int32), rd.view(np.int32))
    emit = G.schedule(calls, 1, lag)[1]                          # with lag >= F every commit happens in the drain
    assert np.array_equal(emit[emit >= 0], np.arange(F)) and np.all(choice[emit < 0] == -1)
    assert np.all(choice[:min(lag, F)] == -1)                    # the warm-up
    got = choice[emit >= 0]
    dsel = dist[np.arange(F), (idx != got[:, None]).argmin(1)].astype(np.float64).sum()
    D = np.array([O.sq_dist(mu[next_of[got[t - 1]]][None], mu[got[t]][None])[0, 0] for t in range(1, F)], np.float64).sum()
    if lag == 0:
        want = LO.greedy(ri, rd, mu, next_of, w)[1]
        assert np.array_equal(got, want) and dsel + w * D == 12.9375 and G.switches(got, F) == F - 1
    else:
        want = P.best_path(ri, rd, mu, next_of, w)[1]
        assert np.array_equal(got, want) and dsel + w * D == 10.5625 and G.switches(got, F) == 1


def test_choices_follow_the_oracle_at_the_default_model_shape():
    M = _M()
    m = _model(1024, 2048, 256, seed=1)
    index = _index(m, 256, lengths=(9000, 20000, 5000))
    sm = M.StreamingMosaic(index, 2, 1024, hop=256, k=16, mode="decode", window="hann", continuity=0.25, lag=6)
    x = _signal(np.random.default_rng(8), 2, 1024 * 5)
    y, idx, dist, choice, calls = [t.cpu().numpy() if torch.is_tensor(t) else t for t in _run(sm, x)]
    assert calls == "pppppddd"
    for s in range(2):
        want, emit, committed = _expected(index, sm, idx[s], dist[s], calls, lambda c: 0.25)
        assert np.array_equal(choice[s], want), np.argwhere(choice[s] != want)[:5]
        ref = _played(index, sm, emit, committed, "decode", "hann")
        assert np.array_equal(y[s].view(np.int32), ref.view(np.int32))


def test_cli_lag_writes_what_the_api_gives(tmp_path):
    from rawvae.model import VAE
    from rawaudiovae_kelsey_amd import data as D
    sys.path.insert(0, REPO)
    S, H, L, sr = 64, 128, 8, 8000
    torch.manual_seed(3)
    model = VAE(S, H, L)
    torch.save({"epoch": 1, "state_dict": model.state_dict(), "optimizer": {}}, tmp_path / "ckpt_00001")
    (tmp_path / "tiny.ini").write_text("[audio]\nsampling_rate = %d\nhop_length = 8\nsegment_length = %d\n"
                                       "[VAE]\nlatent_dim = %d\nn_units = %d\n" % (sr, S, L, H))
    corpus = tmp_path / "corpus"
    corpus.mkdir()
    rng = np.random.default_rng(4)
    waves = _waves(rng, [400, 777, 1024])
    for i, w in enumerate(waves):
        D.write_wav(corpus / ("c%d.wav" % i), w, sr)
    target = (0.3 * rng.standard_normal(999)).astype(np.float32)
    D.write_wav(tmp_path / "t.wav", target, sr)
    lag, block = 5, 64
    run = [sys.executable, os.path.join(REPO, "mosaic.py"), "--config", str(tmp_path / "tiny.ini"), "--checkpoint",
           str(tmp_path / "ckpt_00001"), "--corpus", str(corpus), "--target", str(tmp_path / "t.wav"), "--out",
           str(tmp_path / "out.wav"), "--hop", "16", "--k", "3", "--mode", "grains", "--window", "hann", "--live-block",
           str(block), "--continuity", "0.5", "--lag", str(lag), "--matches", str(tmp_path / "m.csv")]
    r = subprocess.run(run, check=True, timeout=300, cwd=str(tmp_path), capture_output=True, text=True)
    assert ", live, lag 5, block 64, streams 1, continuity 0.5, continuing " in r.stdout and "greedy" not in r.stdout
    y, got_sr = D.read_wav(tmp_path / "out.wav")
    assert got_sr == sr and y.size == target.size
    index = _M().LatentIndex(model.cuda().eval(), hop=16)
    for i, w in enumerate(waves):
        index.add(w, "c%d.wav" % i)
    sm = _M().StreamingMosaic(index, 1, block, hop=16, k=3, mode="grains", window="hann", continuity=0.5, lag=lag)
    n_blocks = -(-(target.size + sm.latency) // block)
    x = np.zeros((1, n_blocks * block), np.float32)
    x[0, :target.size] = target
    calls = "p" * n_blocks + "d" * -(-sm.lag_samples // block)
    out = _run(sm, torch.from_numpy(x).cuda(), calls=calls)
    late = sm.latency + sm.lag_samples
    want = out[0][0, late:late + target.size].cpu().numpy()
    assert np.array_equal(y, want) and np.abs(y).max() > 0
    # --matches pairs every committed choice with its own frame's candidates: the slot is where the choice sits in them
    idx, choice = out[1][0].cpu().numpy(), out[3][0].cpu().numpy()[lag:lag + n_blocks * 4]
    lines = (tmp_path / "m.csv").read_text().strip().split("\n")
    assert len(lines) == n_blocks * 4
    slots = np.array([int(l.split(",")[-1]) for l in lines])
    assert np.all(choice >= 0) and np.array_equal(idx[np.arange(len(slots)), slots], choice)
