"""Latent interpolation (rawaudiovae_kelsey_amd/interpolate.py, interpolate.py, csrc/resynth.hip): the host rules and the
CLI, without a GPU.  Length matching and framing are checked against a restatement of the notebook's match_audio_size
(tutorial.ipynb:423-437) and against the reference datasets' frames in tests/golden/dataset_frames.npz."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, REPO

import interpolate as cli  # noqa: E402  (the entry point at the repository root)
from rawaudiovae_kelsey_amd import _lib, frontend  # noqa: E402
from rawaudiovae_kelsey_amd import interpolate as I  # noqa: E402


def notebook_match(a, b, match_size):
    """match_audio_size restated: 0 crops the longer, 1 doubles the shorter until it is long enough, then crops."""
    if match_size == 0:
        if a.shape[0] < b.shape[0]:
            b = b[:a.shape[0]]
        else:
            a = a[:b.shape[0]]
    else:
        if a.shape[0] < b.shape[0]:
            while a.shape[0] < b.shape[0]:
                a = np.concatenate((a, a), 0)
            a = a[:b.shape[0]]
        else:
            while b.shape[0] < a.shape[0]:
                b = np.concatenate((b, b), 0)
            b = b[:a.shape[0]]
    return a, b


def device_rule(src, n_valid, n_out):
    """What rv_match_pad writes: src[i % n_src] below n_valid, zeros up to n_out."""
    i = np.arange(n_out)
    return np.where(i < n_valid, src[i % len(src)], 0).astype(src.dtype)


@pytest.mark.parametrize("na,nb", [(1000, 2345), (2345, 1000), (640, 640), (3, 1000), (999, 1000), (1, 7)])
@pytest.mark.parametrize("mode,size", [("repeat", 1), ("crop", 0)])
def test_match_length_is_the_notebooks(na, nb, mode, size):
    a = np.arange(na, dtype=np.float32) + 0.5
    b = -np.arange(nb, dtype=np.float32) - 0.25
    ra, rb = notebook_match(a, b, size)
    n = I.matched_length(na, nb, mode)
    assert n == len(ra) == len(rb)
    np.testing.assert_array_equal(device_rule(a, n, n), ra)
    np.testing.assert_array_equal(device_rule(b, n, n), rb)


def test_match_mode_is_checked():
    with pytest.raises(ValueError, match="match mode"):
        I.matched_length(3, 4, "pad")


def test_frame_layout_matches_the_reference_datasets():
    fx = np.load(os.path.join(GOLDEN, "dataset_frames.npz"))
    ramp = np.arange(1000, dtype=np.float32)
    w2 = np.random.default_rng(int(fx["rand_wave_seed"])).uniform(-1, 1, 5000).astype(np.float32)
    for wave, S, hop, hop_key, eval_key in ((ramp, 256, 64, "ramp_hop_frames", "ramp_eval_frames"),
                                            (w2, 512, 128, "rand_hop_frames", "rand_eval_frames")):
        for h, key in ((hop, hop_key), (None, eval_key)):
            n, padded = I.frame_layout(len(wave), S, h)
            assert n == fx[key].shape[0]
            # the padded waveform rv_match_pad builds, framed through the encoder's leading dimension
            buf = device_rule(wave, len(wave), padded)
            step = S if h is None else h
            frames = buf[np.arange(n)[:, None] * step + np.arange(S)[None, :]]
            np.testing.assert_array_equal(frames, fx[key])
            assert (n - 1) * step + S <= padded      # the last frame ends inside the padded waveform


def test_frame_layout_rules():
    assert I.frame_layout(10, 64) == (1, 64)              # shorter than a frame: one zero-padded frame
    assert I.frame_layout(128, 64) == (2, 128)
    assert I.frame_layout(129, 64, 8) == (10, 136)
    assert I.frame_layout(10, 64, 8)[0] < 1                # AudioDataset makes no frame of it (the API refuses)
    with pytest.raises(ValueError, match="not a multiple of hop_size"):
        I.frame_layout(1000, 64, 12)


def test_alpha_specs():
    np.testing.assert_array_equal(cli.parse_alphas("0:1.1:0.2"), np.arange(0, 1.1, 0.2))
    np.testing.assert_array_equal(cli.parse_alphas("0,0.5,1"), [0.0, 0.5, 1.0])
    assert cli.parse_alphas("1:0:-0.25").tolist() == [1.0, 0.75, 0.5, 0.25]
    for bad in ("0:1", "a:b:c", "0:1:0", "", "1:0:0.1", "0,x"):
        with pytest.raises(ValueError, match="--alphas"):
            cli.parse_alphas(bad)


def test_curve_specs(tmp_path):
    c = cli.parse_curve("sin:-500:500:20000")
    np.testing.assert_array_equal(c, np.sin(np.linspace(-500 * np.pi, 500 * np.pi, 20000)))
    assert c.dtype == np.float64
    p = tmp_path / "c.npy"
    np.save(p, np.linspace(0, 1, 5, dtype=np.float32))
    np.testing.assert_array_equal(cli.parse_curve(str(p)), np.linspace(0, 1, 5, dtype=np.float32).astype(np.float64))
    np.save(tmp_path / "flat.npy", np.zeros((2, 3)))
    for bad in ("cos:0:1:10", "sin:0:1", "sin:0:1:1", "sin:a:1:10", str(tmp_path / "missing.npy"),
                str(tmp_path / "flat.npy")):
        with pytest.raises(ValueError, match="--curve"):
            cli.parse_curve(bad)


def test_cli_flags_are_validated():
    base = ["--checkpoint", "c", "--a", "a.wav", "--b", "b.wav", "--out", "o.wav"]
    args = cli.parse_args(base + ["--mode", "curve", "--curve", "sin:-1:1:100", "--hop", "128", "--match", "crop"])
    assert args.hop == 128 and args.match == "crop" and args.curve_values.size == 100 and args.alpha_values is None
    args = cli.parse_args(base)
    assert args.hop is None and args.seed == 0 and args.mode == "stepwise" and args.alpha_values.size == 6
    for flags, name in ((["--mode", "mix"], "--mode"), (["--match", "pad"], "--match"), (["--hop", "x"], "--hop"),
                        (["--hop", "0"], "--hop"), (["--seed", "-1"], "--seed"), (["--max-rows", "0"], "--max-rows"),
                        (["--alphas", "0:1"], "--alphas"), (["--mode", "curve", "--curve", "x"], "--curve")):
        with pytest.raises(ValueError, match=re.escape(name)):
            cli.parse_args(base + flags)
    with pytest.raises(ValueError, match="--config"):
        frontend.read_model_config(os.path.join(REPO, "no_such.ini"))


def test_model_shape_comes_from_the_ini():
    cfg = frontend.read_model_config(os.path.join(REPO, "default.ini"))
    assert cfg == dict(sampling_rate=44100, segment_length=1024, n_units=2048, latent_dim=256)


def test_new_header_entries_compile_as_c(tmp_path):
    """rv_match_pad / rv_latent_mix and the RV_ALPHA_* modes are plain C, and _lib's constants are the header's."""
    if not shutil.which("gcc"):
        pytest.skip("gcc not available")
    src = tmp_path / "mix.c"
    src.write_text('#include "rawvae_hip.h"\n#include <stdio.h>\n'
                   'int main(void) {\n'
                   '  int (*m)(const float*, const float*, const float*, const float*, long, long, int, const void*, long,\n'
                   '           long, long, const float*, float*, unsigned long long, unsigned long long, float*, float*,\n'
                   '           float*, double*, void*) = rv_latent_mix;\n'
                   '  int (*p)(const float*, long, long, float*, long, void*) = rv_match_pad;\n'
                   '  printf("%d %d %d %d %d\\n", RV_ALPHA_LIST, RV_ALPHA_F32, RV_ALPHA_F64, RV_ALPHA_CURVE,\n'
                   '         (m != 0) + (p != 0));\n  return 0;\n}\n')
    obj = tmp_path / "mix.o"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-c", "-I", os.path.join(REPO, "include"), str(src), "-o",
                    str(obj)], check=True)
    hdr = open(os.path.join(REPO, "include", "rawvae_hip.h")).read()
    consts = {k: int(v) for k, v in re.findall(r"#define RV_ALPHA_(\w+) (\d+)", hdr)}
    assert consts == {"LIST": _lib.ALPHA_LIST, "F32": _lib.ALPHA_F32, "F64": _lib.ALPHA_F64, "CURVE": _lib.ALPHA_CURVE}
    assert {"rv_match_pad", "rv_latent_mix"} <= set(_lib.EXPORTED)


def test_interp_fixture_is_complete():
    fx = np.load(os.path.join(GOLDEN, "interp_f32.npz"))
    S, H, L = fx["shape"].tolist()
    K = fx["alphas"].size
    n = max(fx["a"].size, fx["b"].size)
    n_s, _ = I.frame_layout(n, S)
    n_e, _ = I.frame_layout(n, S, S // 8)
    assert fx["out_step"].size == K * n_s * S and fx["eps_step"].shape == (K * n_s, L)
    assert fx["out_curve"].size == n_s * S and fx["out_ext"].size == n_e * S
    assert fx["curve"].dtype == np.float64 and fx["out_ext"].dtype == np.float32
