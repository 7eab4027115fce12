"""GPU parity of the SNAC 24 kHz encoder + residual vector quantiser (HIP, fp32) against the
torch-fp32 CPU restatement (tests/_snac_encoder_ref.py), on synthetic weights and seeded
sine + noise audio.

Bars.  Latent: the decoder's, on a signal of the same O(1) scale: RMS < 1e-4, max |d| < 1e-3.
Codes: a differing code is excused only when the restatement's cosine similarity of its own pick
exceeds that of the device's pick by less than a margin -- 1e-4 for the quantiser alone on the
restatement's z (only fp32 summation order separates the two; a 768-term dot is good to ~5e-5
relative), 1e-2 end to end (10x the latent's max bar; the project's token tie margin) -- and
positions under an excused coarser code are not compared.  Excused + uncompared positions are
capped at 2 % of a run's code positions.

Shapes this file runs (tests/_coverage.py declares the existing files' runs; these are declared
here): latent at 2,048 / 5,000 / 26,624 samples (1, 3, 13 frames), quantiser and encode at
24 frames (49,152 samples), the largest input.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import _snac_encoder_ref as R
from project_morpheus_amd.weights import (snac_shapes, synthetic_snac_encoder_weights,
                                          synthetic_snac_weights)

pytestmark = pytest.mark.gpu

RUN_SAMPLES = {"latent": (2048, 5000, 13 * 2048), "codes": (24 * 2048,)}
MAX_FRAMES = 24


@pytest.fixture(scope="module")
def weights():
    return {**synthetic_snac_weights(seed=3), **synthetic_snac_encoder_weights(seed=5)}


@pytest.fixture(scope="module")
def enc(weights):
    from project_morpheus_amd.engine import SnacEncoder
    e = SnacEncoder(weights, device=0, max_frames=MAX_FRAMES)
    yield e
    e.close()


@pytest.fixture(scope="module")
def ref24(weights):
    """The restatement's run on the 24-frame input, computed once: (audio, frames, trace, z)."""
    audio = R.make_audio(24 * 2048, seed=21)
    frames, _codes, trace, z = R.encode(weights, audio)
    return audio, frames, trace, z


@pytest.mark.parametrize("n_samples", RUN_SAMPLES["latent"])
def test_latent_parity(enc, weights, n_samples):
    """1 frame: 4 latents, every dilated halo wider than the signal at the deepest level; 5,000
    samples: padded to 3 frames; 13 frames: 52 latents, ragged column tiles at every level."""
    audio = R.make_audio(n_samples, seed=n_samples)
    want = R.latent(weights, audio).t().contiguous().numpy()        # [4N][768]
    got = enc.latent(audio)
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    assert got.shape == want.shape == (4 * -(-n_samples // 2048), 768)
    d = got - want
    rms, mx = float(np.sqrt(np.mean(d ** 2))), float(np.abs(d).max())
    print(f"latent n={n_samples}: z RMS {np.sqrt(np.mean(want ** 2)):.3f} diff RMS {rms:.3e} "
          f"max {mx:.3e}")
    assert rms < 1e-4, rms
    assert mx < 1e-3, mx


def _check_codes(tag, ref_frames, dev_frames, trace, margin):
    exact, excused, skipped, fails = R.excused_mismatches(ref_frames, dev_frames, trace, margin)
    total = ref_frames.numel()
    print(f"{tag}: {exact} of {total} codes agree exactly, {excused} excused, {skipped} under an "
          f"excused coarser code")
    assert not fails, fails
    assert exact + excused + skipped == total
    assert excused + skipped <= 0.02 * total, (excused, skipped, total)


def test_quantiser_alone(enc, ref24):
    _audio, frames, trace, z = ref24
    got = enc.quantize(z.t().contiguous())
    torch.cuda.synchronize()
    _check_codes("quantize 24 frames", frames, got.cpu(), trace, 1e-4)


def test_encode_end_to_end(enc, ref24):
    audio, frames, trace, _z = ref24
    got = enc.encode(audio)
    torch.cuda.synchronize()
    assert got.shape == (24, 7) and got.dtype == torch.int32
    _check_codes("encode 24 frames", frames, got.cpu(), trace, 1e-2)


def test_padding_is_zeros_on_the_right(enc):
    audio = R.make_audio(5000, seed=5)
    padded = np.concatenate([audio, np.zeros(3 * 2048 - 5000, np.float32)])
    a = enc.encode(audio)
    b = enc.encode(padded)
    za, zb = enc.latent(audio), enc.latent(padded)
    torch.cuda.synchronize()
    assert a.shape == b.shape == (3, 7)
    assert torch.equal(a, b)
    assert torch.equal(za, zb)


def test_deterministic(enc, ref24):
    audio = ref24[0]
    f1, z1 = enc.encode(audio), enc.latent(audio)
    f2, z2 = enc.encode(audio), enc.latent(audio)
    torch.cuda.synchronize()
    assert torch.equal(f1, f2)
    assert z1.cpu().numpy().tobytes() == z2.cpu().numpy().tobytes()


def test_int16_pcm_input(enc):
    pcm = (R.make_audio(4096, seed=9) * 32768.0).astype(np.int16)
    a = enc.encode(torch.from_numpy(pcm))
    b = enc.encode(pcm.astype(np.float32) / 32768.0)
    torch.cuda.synchronize()
    assert torch.equal(a, b)


def test_codes_in_range_and_decodable(enc, weights, ref24):
    from project_morpheus_amd.engine import SnacDecoder
    frames = enc.encode(ref24[0][:7 * 2048])
    torch.cuda.synchronize()
    assert frames.shape == (7, 7)
    assert int(frames.min()) >= 0 and int(frames.max()) <= 4095
    dec = SnacDecoder({k: weights[k] for k in snac_shapes()}, device=0, max_frames=7)
    pcm, audio = dec.decode(frames.reshape(1, 49), want_audio=True)
    torch.cuda.synchronize()
    assert audio.shape == (1, 7 * 2048) and bool(torch.isfinite(audio).all())
    dec.close()


def test_refusals_enqueue_nothing(enc, weights):
    from project_morpheus_amd import _lib
    lib = enc.lib
    st = torch.cuda.current_stream(0)
    sp = C.c_void_p(st.cuda_stream)
    audio = torch.from_numpy(R.make_audio((MAX_FRAMES + 1) * 2048, seed=2)).cuda()
    SENT = -7
    out = torch.full((MAX_FRAMES + 1, 7), SENT, dtype=torch.int32, device="cuda")
    ap, op = C.c_void_p(audio.data_ptr()), C.c_void_p(out.data_ptr())
    torch.cuda.synchronize()

    def refused(rc, want, handle, word):
        assert rc == want, rc
        assert word in lib.mx_snac_enc_last_error(handle).decode()
        torch.cuda.synchronize()
        assert bool((out == SENT).all()), "a refused call wrote frames"

    # more than max_frames; no samples; a negative count
    refused(lib.mx_snac_enc_encode(enc.h, ap, MAX_FRAMES * 2048 + 1, op, sp), _lib.MX_ERR_ARG,
            enc.h, "max_frames")
    refused(lib.mx_snac_enc_encode(enc.h, ap, 0, op, sp), _lib.MX_ERR_ARG, enc.h, "n_samples")
    refused(lib.mx_snac_enc_encode(enc.h, ap, -5, op, sp), _lib.MX_ERR_ARG, enc.h, "n_samples")
    refused(lib.mx_snac_enc_latent(enc.h, ap, 0, op, sp), _lib.MX_ERR_ARG, enc.h, "n_samples")
    refused(lib.mx_snac_enc_quantize(enc.h, ap, MAX_FRAMES + 1, op, sp), _lib.MX_ERR_ARG, enc.h,
            "n_frames")
    # encode before finalize
    h = C.c_void_p()
    assert lib.mx_snac_enc_create(0, 4, C.byref(h)) == 0
    try:
        refused(lib.mx_snac_enc_encode(h, ap, 2048, op, sp), _lib.MX_ERR_STATE, h, "finalized")
        assert lib.mx_snac_enc_finalize(h) == _lib.MX_ERR_STATE       # weights missing
        assert "missing" in lib.mx_snac_enc_last_error(h).decode()
    finally:
        lib.mx_snac_enc_destroy(h)
    # a good call afterwards passes, on the context that refused
    assert lib.mx_snac_enc_encode(enc.h, ap, MAX_FRAMES * 2048, op, sp) == 0
    torch.cuda.synchronize()
    got = out[:MAX_FRAMES]
    assert int(got.min()) >= 0 and int(got.max()) <= 4095
    assert bool((out[MAX_FRAMES] == SENT).all())
    with pytest.raises(_lib.MxError) as ei:
        enc.encode(audio)
    assert ei.value.rc == _lib.MX_ERR_ARG
