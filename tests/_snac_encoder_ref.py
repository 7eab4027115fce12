"""Torch CPU restatement of the SNAC 24 kHz encoder + residual vector quantiser (TEST
INFRASTRUCTURE, the encoder-side twin of oracle/snac_ref.py).

snac 1.2.x, 24 kHz configuration (encoder_rates [2,4,8,8], encoder_dim 48, latent 768,
vq_strides [4,2,1], codebook 4096 x 8, depthwise, no attention block):

  encode(audio[1,1,T]): T right-padded with zeros to a multiple of 2048
  Encoder: conv k7 pad 3 (1 -> 48); 4 x EncoderBlock(s = 2,4,8,8); depthwise conv k7 pad 3 (768)
  EncoderBlock(s), C channels on entry: ResidualUnit(d = 1,3,9) -> Snake(C)
                   -> Conv1d(C -> 2C, k = 2s, stride s, pad ceil(s/2))
  ResidualUnit(d): x + conv1x1(Snake(dwconv_k7_dil_d(Snake(x))))
  ResidualVectorQuantize: res = z; per level i (stride 4,2,1): r = avg_pool1d(res, stride);
    e = in_proj_i(r); en, cn = F.normalize(e), F.normalize(codebook_i);
    dist = |en|^2 - 2 en cn^T + |cn|^2; code = argmax(-dist) (smallest index on ties);
    zq = repeat_interleave(out_proj_i(codebook_i[code]), stride); res -= zq

Weight norm is folded by the loader (project_morpheus_amd.weights).  The arithmetic runs in
the dtype of the weights handed in (fp32 for parity, fp64 for the reference's own error).

PARITY UNPINNED against snac itself (package and weights absent): the restatement is pinned
only structurally (tests/test_snac_encoder_ref.py).
"""
from __future__ import annotations

import math
from typing import Dict, List, Tuple

import numpy as np
import torch
import torch.nn.functional as F

ENC_RATES = (2, 4, 8, 8)
STRIDES = (4, 2, 1)
DILATIONS = (1, 3, 9)
HOP = 2048  # 512 * lcm(4, 2, 1) samples per frame
# slot of each code inside a 7-code frame: c0[f], c1[2f], c2[4f], c2[4f+1], c1[2f+1], c2[4f+2], c2[4f+3]
FRAME_SLOTS = ((0, 0), (1, 0), (2, 0), (2, 1), (1, 1), (2, 2), (2, 3))


def snake(x: torch.Tensor, alpha: torch.Tensor) -> torch.Tensor:
    a = alpha.reshape(1, -1, 1)
    return x + (a + 1e-9).reciprocal() * torch.sin(a * x).pow(2)


def pad_audio(audio: torch.Tensor) -> torch.Tensor:
    """[..., T] -> [..., ceil(T / 2048) * 2048], zeros on the right only."""
    t = audio.shape[-1]
    return F.pad(audio, (0, math.ceil(t / HOP) * HOP - t))


def encoder(p: Dict[str, torch.Tensor], audio: torch.Tensor) -> torch.Tensor:
    """audio [1, 1, T] (T a multiple of 2048) -> z [1, 768, T / 512]."""
    x = F.conv1d(audio, p["enc.in.w"], p["enc.in.b"], padding=3)
    for k, s in enumerate(ENC_RATES):
        c = x.shape[1]
        for j, d in enumerate(DILATIONS):
            q = f"enc.b{k}.r{j}."
            y = snake(x, p[q + "alpha1"])
            y = F.conv1d(y, p[q + "dw.w"], p[q + "dw.b"], padding=3 * d, dilation=d, groups=c)
            y = snake(y, p[q + "alpha2"])
            y = F.conv1d(y, p[q + "pw.w"].unsqueeze(-1), p[q + "pw.b"])
            x = x + y
        x = snake(x, p[f"enc.b{k}.alpha"])
        x = F.conv1d(x, p[f"enc.b{k}.down.w"], p[f"enc.b{k}.down.b"], stride=s,
                     padding=math.ceil(s / 2))
    return F.conv1d(x, p["enc.out.dw.w"], p["enc.out.dw.b"], padding=3, groups=x.shape[1])


def quantize(p: Dict[str, torch.Tensor], z: torch.Tensor):
    """z [1, 768, 4N] -> (codes [c0 [N], c1 [2N], c2 [4N]] int64, trace).

    ``trace[i]`` = (en [Ti, 8], cn [4096, 8]): the normalised encodings and codebook of level i,
    from which a test reads the cosine similarity of any candidate code."""
    res = z
    codes, trace = [], []
    for i, st in enumerate(STRIDES):
        r = F.avg_pool1d(res, st, st) if st > 1 else res
        e = F.conv1d(r, p[f"q{i}.in_proj.w"].unsqueeze(-1), p[f"q{i}.in_proj.b"])
        en = F.normalize(e[0].t())                      # [Ti, 8]
        cb = p[f"q{i}.codebook"]
        cn = F.normalize(cb)
        dist = en.pow(2).sum(1, keepdim=True) - 2 * en @ cn.t() + cn.pow(2).sum(1, keepdim=True).t()
        code = (-dist).max(1)[1]
        zq = F.conv1d(cb[code].t().unsqueeze(0), p[f"q{i}.out_proj.w"].unsqueeze(-1),
                      p[f"q{i}.out_proj.b"])
        res = res - zq.repeat_interleave(st, dim=-1)
        codes.append(code)
        trace.append((en, cn))
    return codes, trace


def interleave(c0, c1, c2) -> torch.Tensor:
    """c0 [N], c1 [2N], c2 [4N] -> frames [N, 7] int32 in speechpipe order."""
    c = (torch.as_tensor(c0), torch.as_tensor(c1), torch.as_tensor(c2))
    n = c[0].numel()
    out = torch.empty(n, 7, dtype=torch.int32)
    for k, (lvl, off) in enumerate(FRAME_SLOTS):
        per = 1 << lvl
        out[:, k] = c[lvl].reshape(n, per)[:, off].to(torch.int32)
    return out


def code_position(frame: int, k: int) -> Tuple[int, int]:
    """(level, index inside the level's code sequence) of slot k of a frame."""
    lvl, off = FRAME_SLOTS[k]
    return lvl, (frame << lvl) + off


def latent(p: Dict[str, torch.Tensor], audio) -> torch.Tensor:
    """mono samples [T] -> z [768, 4 * ceil(T / 2048)] in the dtype of the weights."""
    dt = p["enc.in.w"].dtype
    a = torch.as_tensor(np.asarray(audio)).to(dt).reshape(1, 1, -1)
    with torch.no_grad():
        return encoder(p, pad_audio(a))[0]


def encode(p: Dict[str, torch.Tensor], audio):
    """mono samples [T] -> (frames [N, 7] int32, codes, trace, z [768, 4N])."""
    with torch.no_grad():
        z = latent(p, audio)
        codes, trace = quantize(p, z.unsqueeze(0))
    return interleave(*codes), codes, trace, z


def to_dtype(p: Dict[str, torch.Tensor], dtype) -> Dict[str, torch.Tensor]:
    return {k: v.to(dtype) for k, v in p.items()}


def make_audio(n_samples: int, seed: int = 11) -> np.ndarray:
    """Seeded sines + noise of amplitude ~0.3, float32 mono."""
    rng = np.random.default_rng(seed)
    t = np.arange(n_samples, dtype=np.float64) / 24000.0
    x = 0.18 * np.sin(2 * np.pi * 220.0 * t) + 0.09 * np.sin(2 * np.pi * 1370.0 * t + 0.7)
    x += 0.03 * rng.standard_normal(n_samples)
    return x.astype(np.float32)



def excused_mismatches(frames_ref: torch.Tensor, frames_dev: torch.Tensor, trace,
                       margin: float) -> Tuple[int, int, int, List[str]]:
    """Compare two [N, 7] frame tensors under the near-tie rule.

    A differing code is excused when the restatement's cosine similarity of its own pick
    exceeds that of the device's pick by less than ``margin``.  Finer-level positions under a
    differing coarser code are not compared (their residual legitimately differs).
    -> (exact agreements, excused, skipped, inexcusable descriptions)."""
    n = frames_ref.shape[0]
    bad0 = set()   # frames whose level-0 code differs
    bad1 = set()   # level-1 indices whose code (or the level-0 code above) differs
    exact = excused = skipped = 0
    fails: List[str] = []
    order = sorted(range(7), key=lambda k: FRAME_SLOTS[k][0])
    for f in range(n):
        for k in order:
            lvl, idx = code_position(f, k)
            if (lvl >= 1 and f in bad0) or (lvl == 2 and (idx >> 1) in bad1):
                skipped += 1
                continue
            a, b = int(frames_ref[f, k]), int(frames_dev[f, k])
            if a == b:
                exact += 1
                continue
            en, cn = trace[lvl]
            gap = float(en[idx] @ cn[a] - en[idx] @ cn[b]) if 0 <= b < 4096 else float("inf")
            if gap < margin:
                excused += 1
            else:
                fails.append(f"frame {f} slot {k}: ref {a} dev {b} cosine gap {gap:.3e}")
            if lvl == 0:
                bad0.add(f)
            elif lvl == 1:
                bad1.add(idx)
    return exact, excused, skipped, fails
