"""Per-GPU synthesis service: weights -> LlmEngine + SnacDecoder + a continuous-batching loop.

The reference keeps one cached model per process behind an asyncio.Lock + lru_cache
(llama_local.py:35-59) and, on its GPU path, hands every request to vLLM's continuous batcher
from its own thread (Orpheus-TTS/orpheus_tts_pypi/orpheus_tts/engine_class.py:114-134).  Here
one ``Service`` per GPU process owns the engine and a ``BatchSynthesizer`` running online:
concurrent adapters ``submit`` streams that join the batch as they arrive (no lock, no
one-slot serialisation); ``cancel`` (barge-in) frees the stream's KV row.  Several GPUs are
served by ``dispatch.GpuPool`` (one worker process per GPU, least-loaded assignment).

Generation parameters follow the reference's module globals at call time
(``inference.TEMPERATURE / TOP_P / MAX_TOKENS``, updated by ``update_generation_params``,
inference.py:75-105) with the fixed repetition penalty 1.1.
"""
from __future__ import annotations

import queue
import threading
import warnings
from typing import Iterator, Optional

import numpy as np
import torch

from . import config as C
from . import inference as I
from .batching import (BatchSynthesizer, StreamHandle, StreamRequest, UnknownPrefix,
                       check_prefix)
from .engine import SAMPLES_PER_FRAME, LlmEngine, SnacDecoder, SnacEncoder
from .tokenizer import Tokenizer, default_tokenizer
from .weights import (load_hf_llm, load_snac_state_dict, synthetic_llm_weights,
                      synthetic_snac_encoder_weights, synthetic_snac_weights)

VOICE_MAX_FRAMES = 384  # 32 s of reference audio: the largest encoder context a service builds


class Service:
    def __init__(self, device: int = C.MX_DEVICE, cfg: Optional[C.OrpheusConfig] = None,
                 llm_weights=None, snac_weights=None, max_pos: int = 2048,
                 tokenizer: Optional[Tokenizer] = None, max_prefill: int = 512,
                 max_batch: int = C.MX_MAX_SLOTS, synthetic_audio: Optional[bool] = None,
                 packed_prefill: Optional[bool] = None, prefix_slots: Optional[int] = None,
                 snac_encoder_weights=None):
        """``snac_encoder_weights``: the SNAC encoder's weights (``weights.snac_encoder_shapes``)
        for ``register_voice`` / ``encode_audio``; None: from MORPHEUS_MX_SNAC, synthetic when
        unset.  The encoder is built at first use, nothing is allocated for it before.
        ``prefix_slots``: template KV slots for registered prefixes (``register_prefix``;
        None: MORPHEUS_MX_PREFIX_SLOTS, 0 when unset -- nothing is allocated for them then).
        ``synthetic_audio``: feed the SNAC schedule a seeded audio-code stream per request
        (default: whenever the LLM weights are synthetic, which never speak).
        ``packed_prefill``: admit the requests of one loop iteration through packed prefills
        (None: MORPHEUS_MX_PACKED_PREFILL, off when unset)."""
        torch.cuda.set_device(device)
        synthetic = False
        if cfg is None:
            cfg = C.OrpheusConfig.from_hf(C.MX_WEIGHTS) if C.MX_WEIGHTS else C.OrpheusConfig()
        if llm_weights is None:
            if C.MX_WEIGHTS:
                llm_weights = load_hf_llm(C.MX_WEIGHTS, device=f"cuda:{device}")
            else:
                warnings.warn("MORPHEUS_MX_WEIGHTS unset: seeded SYNTHETIC Orpheus weights")
                llm_weights = synthetic_llm_weights(cfg, seed=0, device=f"cuda:{device}")
                synthetic = True
        if snac_weights is None:
            snac_weights = load_snac_state_dict(C.MX_SNAC) if C.MX_SNAC else \
                synthetic_snac_weights()
        self.cfg, self.device = cfg, device
        self.synthetic_audio = synthetic if synthetic_audio is None else synthetic_audio
        prefix_slots = C.prefix_slots_default() if prefix_slots is None else int(prefix_slots)
        self.llm = LlmEngine(cfg, llm_weights, device=device, max_slots=max_batch + prefix_slots,
                             max_pos=max_pos, max_batch=max_batch, max_prefill=max_prefill)
        del llm_weights
        self.snac = SnacDecoder(snac_weights, device=device, max_batch=max_batch)
        # the quantiser searches the codebooks the decoder embeds with
        self._vq_weights = {k: v for k, v in snac_weights.items() if k.startswith("q")}
        self._enc_weights = snac_encoder_weights
        self.batch = BatchSynthesizer(self.llm, self.snac, packed_prefill=packed_prefill,
                                      prefix_slots=prefix_slots).start()
        self.tok = tokenizer or default_tokenizer()

    @classmethod
    def from_engines(cls, llm: LlmEngine, snac: SnacDecoder, cfg: C.OrpheusConfig,
                     synthetic_audio: bool, tokenizer: Optional[Tokenizer] = None) -> "Service":
        """A service over engines that already exist (bench: the configs[1] line through the
        shipped adapter -> Service -> BatchSynthesizer path, on the bench's own weights)."""
        self = cls.__new__(cls)
        self.cfg, self.device = cfg, llm.device
        self.synthetic_audio = synthetic_audio
        self.llm, self.snac = llm, snac
        self.batch = BatchSynthesizer(llm, snac).start()
        self.tok = tokenizer or default_tokenizer()
        return self

    @property
    def outstanding_tokens(self) -> int:
        return self.batch.outstanding_tokens

    def prompt_ids(self, text: str, voice: str):
        return I.prompt_ids(self.tok.encode(f"{I.resolve_voice(voice)}: {text}"))

    def register_prefix(self, name: str, ids):
        """Prefill ``ids`` (raw ids, e.g. ``inference.frame_voice_pairs``) once under ``name``;
        requests submitted with ``prefix=name`` continue behind them.  -> a handle
        (``result()`` waits and raises what refused it)."""
        return self.batch.register_prefix(name, ids)

    def unregister_prefix(self, name: str):
        return self.batch.unregister_prefix(name)

    # ------------------------------------------------------------------ voice prompts from audio
    def _voice_encoder(self) -> SnacEncoder:
        """The SNAC encoder, built at first use (call under ``_enc_lock``)."""
        enc = getattr(self, "_enc", None)
        if enc is None:
            w = getattr(self, "_enc_weights", None)
            if w is None:
                if C.MX_SNAC:
                    w = load_snac_state_dict(C.MX_SNAC, encoder=True)
                else:
                    warnings.warn("MORPHEUS_MX_SNAC unset: seeded SYNTHETIC SNAC encoder weights")
                    w = synthetic_snac_encoder_weights()
            vq = getattr(self, "_vq_weights", None) or synthetic_snac_weights()
            w = {**{k: v for k, v in vq.items() if k.startswith("q")}, **w}
            enc = self._enc = SnacEncoder(w, device=self.device, max_frames=self.voice_max_frames)
            self._enc_stream = torch.cuda.Stream(self.device)
        return enc

    @property
    def voice_max_frames(self) -> int:
        """Frames of reference audio one voice prompt may hold: what fits ``max_pos`` as ids,
        at most ``VOICE_MAX_FRAMES``."""
        return max(1, min(VOICE_MAX_FRAMES, (self.llm.max_pos - 9) // 7))

    def _check_audio(self, audio, sample_rate: int) -> int:
        """-> frames the audio encodes to; ValueError on what no encode is tried for."""
        if int(sample_rate) != I.SAMPLE_RATE:
            raise ValueError(f"voice audio must be {I.SAMPLE_RATE} Hz mono, got {sample_rate} Hz "
                             "(there is no resampler)")
        n = int(np.prod(tuple(audio.shape))) if hasattr(audio, "shape") else len(audio)
        if n < 1:
            raise ValueError("voice audio is empty")
        frames = -(-n // SAMPLES_PER_FRAME)
        if frames > self.voice_max_frames:
            raise ValueError(f"voice audio of {frames} frames exceeds {self.voice_max_frames} "
                             f"({self.voice_max_frames * SAMPLES_PER_FRAME / I.SAMPLE_RATE:.1f} s)")
        return frames

    def encode_audio(self, audio, sample_rate: int = I.SAMPLE_RATE):
        """Mono 24 kHz audio (float in [-1, 1] or int16 PCM; numpy or torch, host or device) ->
        its audio-token ids (``inference.audio_ids_from_frames`` of the SNAC encoder's frames).
        Runs in the caller's thread on the encoder's own HIP stream, one encode at a time."""
        self._check_audio(audio, sample_rate)
        with _enc_lock:
            enc = self._voice_encoder()
            frames = enc.encode(audio, stream=self._enc_stream)
            self._enc_stream.synchronize()
        return I.audio_ids_from_frames(frames.cpu())

    def voice_prefix_ids(self, text: str, audio, sample_rate: int = I.SAMPLE_RATE):
        """The framed ids of the voice prompt (text, audio): ``frame_voice_pairs([(text ids,
        audio ids)])``.  ValueError, before anything is encoded, on a sample rate other than
        24,000, empty audio, audio beyond ``voice_max_frames``, or a framed prompt that would
        not fit ``max_pos``."""
        frames = self._check_audio(audio, sample_rate)
        text_ids = self.tok.encode(text)
        if not text_ids:
            raise ValueError("a voice prompt needs its transcript")
        n = len(I.frame_voice_pairs([(text_ids, [0])])) - 1 + 7 * frames
        if n >= self.llm.max_pos - 1:
            raise ValueError(f"voice prompt of {n} ids does not fit (max_pos {self.llm.max_pos}: "
                             "it needs room for a suffix and a token)")
        return I.frame_voice_pairs([(text_ids, self.encode_audio(audio, sample_rate))])

    def register_voice(self, name: str, text: str, audio, sample_rate: int = I.SAMPLE_RATE):
        """Register a cloned voice from a recording and its transcript: encode ``audio``, frame
        it with ``text`` and ``register_prefix`` the result under ``name`` -> that handle.
        Requests then name it with ``submit(prefix=name)``."""
        check_prefix(name)
        if not name:
            raise ValueError("voice name must be a non-empty string")
        if self.batch.prefix_slots < 1:
            raise ValueError("no template slots (prefix_slots is 0)")
        return self.register_prefix(name, self.voice_prefix_ids(text, audio, sample_rate))

    def _check_prefix(self, prefix) -> None:
        """Refused at submit time (ValueError: HTTP 400): a prefix that is no name, or that
        nobody registered here.  (One evicted later fails its request alone, in the loop.)"""
        check_prefix(prefix)
        if prefix is not None and not self.batch.has_prefix(prefix):
            raise UnknownPrefix(f"unknown prefix {prefix!r}")

    def submit(self, text: str, voice: str = I.DEFAULT_VOICE, max_tokens: Optional[int] = None,
               penalty: float = I.REPETITION_PENALTY, temperature: Optional[float] = None,
               top_p: Optional[float] = None, seed: Optional[int] = None,
               prompt_ids=None, top_k: Optional[int] = None, min_p: Optional[float] = None,
               penalty_last_n: Optional[int] = None,
               grammar: Optional[bool] = None, prefix: Optional[str] = None) -> StreamHandle:
        """Queue one utterance on this GPU's batch loop (non-blocking).  ``grammar``: decode
        under the Orpheus code grammar (None: MORPHEUS_MX_GRAMMAR, off when unset).
        ``prefix``: a registered prefix the prompt continues (``register_prefix``)."""
        self._check_prefix(prefix)
        ids = list(prompt_ids) if prompt_ids is not None else self.prompt_ids(text, voice)
        max_tokens = max_tokens or I.MAX_TOKENS
        # one utterance's random streams (sampling, SNAC noise, synthetic codes) come from ONE
        # per-request seed, so its audio never depends on arrival order or batch company;
        # without a seed it is fresh per request (config.request_seed / CONTENT_SEED)
        key = C.request_seed(ids, seed)
        req = StreamRequest(
            prompt_ids=ids, max_tokens=max_tokens, penalty=penalty,
            temperature=I.TEMPERATURE if temperature is None else temperature,
            top_p=I.TOP_P if top_p is None else top_p, seed=key, noise_seed=key,
            top_k=I.TOP_K if top_k is None else top_k,
            min_p=I.MIN_P if min_p is None else min_p,
            penalty_last_n=I.REPEAT_LAST_N if penalty_last_n is None else penalty_last_n,
            grammar=C.grammar_default() if grammar is None else bool(grammar), prefix=prefix,
            inject_ids=C.synthetic_audio_ids(max_tokens, seed=key)
            if self.synthetic_audio else None)
        if self.synthetic_audio:
            req.stop_ids = ()  # synthetic weights decode the full budget (bench contract)
        return self.batch.submit(req)

    def submit_tokens(self, prompt_ids, max_tokens: Optional[int] = None,
                      temperature: Optional[float] = None, top_p: Optional[float] = None,
                      penalty: float = I.REPETITION_PENALTY, seed: Optional[int] = None,
                      top_k: Optional[int] = None, min_p: Optional[float] = None,
                      penalty_last_n: Optional[int] = None, grammar: Optional[bool] = None,
                      prefix: Optional[str] = None):
        """Token-only stream (completions surface): a TokenHandle of generated ids."""
        self._check_prefix(prefix)
        ids = list(prompt_ids)
        key = C.request_seed(ids, seed)
        req = StreamRequest(prompt_ids=ids, max_tokens=max_tokens or I.MAX_TOKENS,
                            penalty=penalty,
                            temperature=I.TEMPERATURE if temperature is None else temperature,
                            top_p=I.TOP_P if top_p is None else top_p, seed=key, audio=False,
                            top_k=I.TOP_K if top_k is None else top_k,
                            min_p=I.MIN_P if min_p is None else min_p,
                            penalty_last_n=I.REPEAT_LAST_N if penalty_last_n is None
                            else penalty_last_n,
                            grammar=C.grammar_default() if grammar is None else bool(grammar),
                            prefix=prefix)
        return self.batch.submit(req)

    def stream(self, text: str, voice: str = I.DEFAULT_VOICE, max_tokens: Optional[int] = None,
               penalty: float = I.REPETITION_PENALTY, stats=None,
               cancel: Optional[threading.Event] = None, **kw) -> Iterator[bytes]:
        """PCM16 chunks of one utterance in order; ``cancel`` (or closing the generator)
        cancels the stream on the GPU and frees its row."""
        h = self.submit(text, voice, max_tokens, penalty, **kw)
        try:
            while True:
                if cancel is not None and cancel.is_set():
                    return
                try:
                    c = h.get(timeout=0.05)
                except queue.Empty:
                    continue
                if c is None:
                    return
                yield c
        finally:
            h.cancel()
            if stats is not None:
                stats.tokens = len(h.req.tokens)
                stats.samples = h.req.samples

    def close(self) -> None:
        self.batch.stop()
        enc = getattr(self, "_enc", None)
        if enc is not None:
            enc.close()


_enc_lock = threading.Lock()   # one voice encode at a time per process
_service: Optional[Service] = None
_service_lock = threading.Lock()


def get_service():
    """The process' synthesis backend: one ``Service`` on this GPU, or a ``GpuPool`` of
    worker processes when MORPHEUS_MX_GPUS > 1 (both expose ``stream`` / ``submit``)."""
    global _service
    with _service_lock:
        if _service is None:
            if C.MX_GPUS > 1:
                from .dispatch import GpuPool
                _service = GpuPool(C.MX_GPUS)
            else:
                _service = Service(max_pos=min(C.MX_MAX_POS, 8192))
        return _service
