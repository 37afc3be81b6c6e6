"""The host layer the audio tools share, on the GPU: FrameCodec (rawaudiovae_kelsey_amd/codec.py) against the model's
own exact-fp32 inference, chunked and into a slice, and the graph capture / replay that StreamingVAE and StreamingMosaic
share (stream.GraphReplay) against the eager calls of a twin, and corpus.encode_corpus against the codec file by file.
Everything bit for bit: the same kernels, every row on its own."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

S, H, L = 64, 96, 8
BEFORE = "%s before capture()"
REPLACED = "a Parameter of the model was replaced after capture(): capture again"


def _model(seed=0):
    from rawvae.model import VAE
    torch.manual_seed(seed)
    return VAE(S, H, L).cuda().eval()


@pytest.fixture(scope="module")
def model():
    return _model()


@pytest.fixture(scope="module")
def codec(model):
    from rawaudiovae_kelsey_amd.codec import FrameCodec
    return FrameCodec(model, max_rows=3)        # 7 rows: chunks of 3, 3 and 1


def _randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).cuda()


def test_encode_in_chunks_equals_the_models_encoder(model, codec):
    w = codec.wave(0.5 * _randn(150, seed=1).cpu().numpy())
    padded, n_frames = codec.pad(w, w.numel(), 16)
    assert (n_frames, padded.numel()) == (7, 160) and list(codec.chunks(7)) == [(0, 3), (3, 3), (6, 1)]
    mu, logvar = codec.encode(padded, n_frames, 16)
    with torch.no_grad():
        want = model.encode(padded.unfold(0, S, 16))
    assert torch.equal(mu, want[0]) and torch.equal(logvar, want[1])


def test_decode_in_chunks_equals_the_models_decoder_and_writes_only_its_slice(model, codec):
    z = _randn(7, L, seed=2)
    with torch.no_grad():
        want = model.decode(z)
    got = codec.decode(z)
    assert got.shape == (7, S) and torch.equal(got, want)
    wave = torch.full((12 * S,), 7.0, device="cuda")                 # tanh never gives the sentinel
    out = wave[2 * S:9 * S]
    assert codec.decode(z, out=out) is out
    assert torch.equal(wave[2 * S:9 * S].view(7, S), want)
    assert bool((wave[:2 * S] == 7.0).all()) and bool((wave[9 * S:] == 7.0).all())
    with pytest.raises(ValueError, match="out must hold"):
        codec.decode(z, out=wave[:6 * S])


def _replace_a_parameter(m):
    m.fc4.weight = torch.nn.Parameter(m.fc4.weight.detach().clone())


def _raises(call, text):
    from rawaudiovae_kelsey_amd._lib import RvError
    with pytest.raises(RvError) as e:
        call()
    assert str(e.value) == text


def test_streaming_vae_replay_equals_the_eager_twin_and_guards_its_parameters():
    from rawaudiovae_kelsey_amd.stream import StreamingVAE
    m = _model()
    eager, graph = (StreamingVAE(m, 2, 32, hop=16, window="hann", seed=3) for _ in range(2))
    _raises(graph.replay, BEFORE % "replay()")
    assert graph.capture() is graph and graph.graph_input.shape == graph.graph_output.shape == (2, 32)
    x = 0.5 * _randn(2, 96, seed=4)
    for b in range(3):
        blk = x[:, 32 * b:32 * b + 32]
        assert torch.equal(graph.replay(blk), eager.process(blk)), b
    _replace_a_parameter(m)
    _raises(graph.replay, REPLACED)
    torch.cuda.synchronize()


def test_streaming_mosaic_replay_and_drain_replay_equal_the_eager_twin_and_guard_the_parameters():
    from rawaudiovae_kelsey_amd.mosaic import LatentIndex, StreamingMosaic
    m = _model()
    index = LatentIndex(m, hop=16)
    t = np.arange(688) / 8000.0
    assert index.add((0.6 * np.sin(2 * np.pi * 320 * t) + 0.2 * _randn(688, seed=5).cpu().numpy()).astype(np.float32),
                     "corpus") == 40
    eager, graph = (StreamingMosaic(index, 2, 32, hop=16, k=2, window="hann", continuity=0.5, lag=2) for _ in range(2))
    _raises(graph.replay, BEFORE % "replay()")
    _raises(graph.drain_replay, BEFORE % "drain_replay()")
    assert graph.capture() is graph
    x = 0.5 * _randn(2, 96, seed=6)
    for b in range(3):
        blk = x[:, 32 * b:32 * b + 32]
        assert torch.equal(graph.replay(blk), eager.process(blk)), b
        assert all(torch.equal(p, q) for p, q in zip(graph.last_matches(), eager.last_matches())), b
    for b in range(graph.drain_blocks):
        assert torch.equal(graph.drain_replay(), eager.drain()), b
    _replace_a_parameter(m)
    _raises(graph.replay, REPLACED)
    _raises(graph.drain_replay, REPLACED)
    torch.cuda.synchronize()


@pytest.mark.parametrize("hop, starts", [(None, [0, 1, 3, 5]), (S // 4, [0, 1, 6, 8])])
def test_encode_corpus_is_the_files_encodings_joined_and_the_three_fits_start_from_it(model, hop, starts):
    """60, 120 and 70 samples: 1, 5 and 2 frames at hop S / 4 (1, 2 and 2 without a hop), every tail zero-padded; with
    max_rows = 4 the 5 frames cross a chunk edge."""
    from rawaudiovae_kelsey_amd import pca as P
    from rawaudiovae_kelsey_amd import states as ST
    from rawaudiovae_kelsey_amd import walk as W
    from rawaudiovae_kelsey_amd.codec import FrameCodec
    from rawaudiovae_kelsey_amd.corpus import encode_corpus
    waves = [0.5 * _randn(n, seed=10 + i).cpu().numpy() for i, n in enumerate((60, 120, 70))]
    codec, want = FrameCodec(model, max_rows=4), []
    for w in waves:
        w = codec.wave(w)
        padded, n_frames = codec.pad(w, w.numel(), hop)
        want.append(codec.encode(padded, n_frames, hop)[0])
    mu, row_start = encode_corpus(model, waves, hop, max_rows=4)
    assert row_start.dtype == np.int64 and row_start.tolist() == starts
    assert mu.shape == (starts[-1], L) and torch.equal(mu, torch.cat(want, 0))
    one, rs = encode_corpus(model, iter(waves[:1]), hop, max_rows=4)
    assert rs.tolist() == [0, 1] and torch.equal(one, want[0])

    pca, by_hand = P.fit_corpus(model, waves, hop, 3, max_rows=4), P.LatentPCA(3).fit(mu)
    for name in ("mean_", "components_", "explained_variance_", "all_variances_"):
        assert torch.equal(getattr(pca, name), getattr(by_hand, name)), name
    walk, by_hand = W.fit_corpus(model, waves, hop, 2, max_rows=4), W.LatentWalk(2).fit(mu, row_start)
    assert walk.row_start_.tolist() == starts and (walk.n_frames_, walk.n_files_) == (starts[-1], 3)
    for name in ("mean_", "components_", "explained_variance_", "dyn_", "P_", "R_", "lagcov_"):
        assert torch.equal(getattr(walk, name), getattr(by_hand, name)), name
    states, by_hand = ST.fit_corpus(model, waves, hop, 2, 2, iters=3, max_rows=4), ST.LatentStates(2, 2)
    history = by_hand.fit(mu, row_start, None, 3)
    assert states.row_start_.tolist() == starts and states.ll_history_ == history
    for name in ("theta_", "mean_", "P_"):
        assert torch.equal(getattr(states, name), getattr(by_hand, name)), name

    for fit in (encode_corpus, P.fit_corpus, W.fit_corpus, ST.fit_corpus):
        with pytest.raises(ValueError) as e:
            fit(model, [], hop)
        assert str(e.value) == "fit_corpus needs at least one waveform"
    with pytest.raises(ValueError) as e:
        W.fit_corpus(model, waves[:1], hop)
    assert str(e.value) == "fit_corpus needs at least 2 frames, the waveforms make 1"
    with pytest.raises(ValueError) as e:
        encode_corpus(model, [waves[0], waves[1][:S // 2]], S // 4)
    assert str(e.value) == "waveform 1: 32 samples make no frame of 64 samples at hop 16"
