"""The host layer the audio tools share, on the GPU: FrameCodec (rawaudiovae_kelsey_amd/codec.py) against the model's
own exact-fp32 inference, chunked and into a slice, and the graph capture / replay that StreamingVAE and StreamingMosaic
share (stream.GraphReplay) against the eager calls of a twin.  Everything bit for bit: the same kernels, every row on
its own."""
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
