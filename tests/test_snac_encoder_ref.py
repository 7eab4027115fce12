"""Structural pins of the SNAC encoder restatement (tests/_snac_encoder_ref.py) and of the host
pieces around it: frame count and padding, the restatement's own fp32 error, the id mapping and
the frame interleave against the decoder-side oracle, and the checkpoint loader's encoder keys.
PARITY UNPINNED against snac itself (package and weights absent): nothing else can be pinned."""
import numpy as np
import pytest
import torch

import _snac_encoder_ref as R
from oracle import speechpipe_ref
from project_morpheus_amd import inference as I
from project_morpheus_amd import schedule
from project_morpheus_amd.weights import (fold_weight_norm, load_snac_state_dict, snac_encoder_shapes,
                                          snac_shapes, synthetic_snac_encoder_weights,
                                          synthetic_snac_weights)


@pytest.fixture(scope="module")
def weights():
    return {**synthetic_snac_weights(seed=3), **synthetic_snac_encoder_weights(seed=5)}


def test_synthetic_weights_have_the_declared_shapes(weights):
    shapes = snac_encoder_shapes()
    assert not set(shapes) & set(snac_shapes())
    for k, shape in shapes.items():
        assert tuple(weights[k].shape) == shape and weights[k].dtype == torch.float32, k
    assert shapes["enc.b3.down.w"] == (768, 384, 16) and shapes["q0.in_proj.w"] == (8, 768)


@pytest.mark.parametrize("n,frames", [(1, 1), (2048, 1), (2049, 2), (5000, 3)])
def test_frames_and_latent_shape(weights, n, frames):
    z = R.latent(weights, R.make_audio(n, seed=n))
    assert z.shape == (768, 4 * frames)
    fr, codes, _, _ = R.encode(weights, R.make_audio(n, seed=n))
    assert fr.shape == (frames, 7) and fr.dtype == torch.int32
    assert [c.numel() for c in codes] == [frames, 2 * frames, 4 * frames]
    assert int(fr.min()) >= 0 and int(fr.max()) <= 4095


def test_padding_is_on_the_right_only(weights):
    a = R.make_audio(5000, seed=1)
    right = np.concatenate([a, np.zeros(3 * 2048 - 5000, np.float32)])
    left = np.concatenate([np.zeros(3 * 2048 - 5000, np.float32), a])
    assert torch.equal(R.latent(weights, a), R.latent(weights, right))
    assert not torch.equal(R.latent(weights, a), R.latent(weights, left))
    assert R.pad_audio(torch.ones(1, 1, 3))[0, 0].tolist() == [1.0] * 3 + [0.0] * 2045


@pytest.mark.parametrize("n", [2048, 5000, 13 * 2048, 24 * 2048])
def test_fp32_restatement_against_fp64(weights, n):
    """The reference alone never flips a code on the GPU tests' inputs."""
    audio = R.make_audio(n, seed=21 if n == 24 * 2048 else n)
    f32, _, _, z32 = R.encode(weights, audio)
    f64, _, _, z64 = R.encode(R.to_dtype(weights, torch.float64), audio)
    assert torch.equal(f32, f64)
    assert float((z32.double() - z64).abs().max()) < 1e-4


def test_audio_ids_round_trip():
    rng = np.random.default_rng(0)
    frames = rng.integers(0, 4096, size=(5, 7)).astype(np.int32)
    ids = I.audio_ids_from_frames(torch.from_numpy(frames))
    assert len(ids) == 35 and ids[0] == 128266 + int(frames[0, 0])
    assert [schedule.code_of_id(t, i) for i, t in enumerate(ids)] == frames.reshape(-1).tolist()
    assert I.audio_ids_from_frames(frames.tolist()) == ids
    for bad in ([[0] * 6], [[0] * 6 + [4096]], [[-1] + [0] * 6]):
        with pytest.raises(ValueError):
            I.audio_ids_from_frames(bad)


def test_interleave_is_the_inverse_of_the_speechpipe_deinterleave():
    n = 3
    c0, c1, c2 = (torch.arange(n) + 100, torch.arange(2 * n) + 200, torch.arange(4 * n) + 300)
    frames = R.interleave(c0, c1, c2)
    d0, d1, d2 = speechpipe_ref.deinterleave(frames.reshape(-1).tolist())
    assert (list(d0), list(d1), list(d2)) == (c0.tolist(), c1.tolist(), c2.tolist())
    assert schedule.deinterleave(frames.reshape(-1).tolist())[2] == c2.tolist()
    for f in range(n):
        for k in range(7):
            lvl, idx = R.code_position(f, k)
            assert int(frames[f, k]) == int((c0, c1, c2)[lvl][idx])


def _encoder_state_dict(sd, w, parametrized):
    """Add the encoder and in_proj entries of a snac 1.2.x state dict for engine weights ``w``."""
    g = torch.Generator().manual_seed(13)
    folds = {}

    def wn(prefix, name, shape=None):
        t = w[name] if shape is None else w[name].reshape(shape)
        gg = 0.5 + torch.rand((t.shape[0],) + (1,) * (t.dim() - 1), generator=g)
        v = torch.randn(t.shape, generator=g)
        a, b = (".parametrizations.weight.original0", ".parametrizations.weight.original1") \
            if parametrized else (".weight_g", ".weight_v")
        sd[prefix + a], sd[prefix + b] = gg, v
        folds[name] = fold_weight_norm(gg, v).reshape(w[name].shape)

    for i in range(3):
        q = f"quantizer.quantizers.{i}.in_proj"
        for k in [k for k in sd if k.startswith(q)]:
            del sd[k]
        wn(q, f"q{i}.in_proj.w", (8, 768, 1))
        sd[q + ".bias"] = w[f"q{i}.in_proj.b"]
    e = "encoder.block."
    wn(e + "0", "enc.in.w")
    sd[e + "0.bias"] = w["enc.in.b"]
    for k in range(4):
        m, p, c = f"{e}{1 + k}.block.", f"enc.b{k}.", 48 << k
        for j in range(3):
            r, q = f"{m}{j}.block.", f"{p}r{j}."
            sd[r + "0.alpha"] = w[q + "alpha1"].reshape(1, -1, 1)
            wn(r + "1", q + "dw.w")
            sd[r + "1.bias"] = w[q + "dw.b"]
            sd[r + "2.alpha"] = w[q + "alpha2"].reshape(1, -1, 1)
            wn(r + "3", q + "pw.w", (c, c, 1))
            sd[r + "3.bias"] = w[q + "pw.b"]
        sd[m + "3.alpha"] = w[p + "alpha"].reshape(1, -1, 1)
        wn(m + "4", p + "down.w")
        sd[m + "4.bias"] = w[p + "down.b"]
    wn(e + "5", "enc.out.dw.w")
    sd[e + "5.bias"] = w["enc.out.dw.b"]
    return folds


@pytest.mark.parametrize("parametrized", [False, True])
def test_loader_maps_the_encoder(tmp_path, weights, parametrized):
    from safetensors.torch import save_file
    from test_checkpoints import _snac_1_2_state_dict
    sd = _snac_1_2_state_dict(weights, parametrized=parametrized)
    folds = _encoder_state_dict(sd, weights, parametrized)
    f = str(tmp_path / "snac.safetensors")
    save_file({k: v.contiguous() for k, v in sd.items()}, f)
    dec = load_snac_state_dict(f)
    assert set(dec) == set(snac_shapes())                      # the default: today's key set
    got = load_snac_state_dict(f, encoder=True)
    shapes = snac_encoder_shapes()
    assert set(got) == set(snac_shapes()) | set(shapes)
    for k, shape in shapes.items():
        assert tuple(got[k].shape) == shape, k
        want = folds[k] if k in folds else weights[k]
        torch.testing.assert_close(got[k], want, rtol=0, atol=0, msg=k)
    for k in dec:
        assert torch.equal(dec[k], got[k]), k
