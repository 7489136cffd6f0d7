"""LLM JSON API -- compatible with app/vllm_model_api.py, app/vllm_model_api_m.py
(multimodal ``image`` field) and app/deepseek_model_api.py.

  POST /generate  {"prompt": str, "max_new_tokens": int, "image"?: base64,
                   "temperature"?, "top_k"?, "top_p"?, "min_p"?, "repetition_penalty"?, "presence_penalty"?,
                   "frequency_penalty"?, "seed"?, "logprobs"?: 0..20,
                   "logit_bias"?: {"<token id>": -100..100}, "allowed_token_ids"?: [int], "min_tokens"?: int,
                   "bad_words"?: [str], "bad_words_ids"?: [[int]], "guided_choice"?: [str],
                   "guided_choice_ids"?: [[int]]}     (strings are tokenised without special tokens)
                  -> {"text": base64(utf-8 text), "execution_time": float,
                      "logprobs"?: [{"token", "logprob", "top_ids", "top_logprobs"}, ...]}   (only when asked)
  POST /benchmark {"n_runs": int, "max_new_tokens": int, "prompt": str}
                  -> {"report": base64("RESULT FOR benchmark:<app> on <nodepool> with <n> output tokens: Latency P0=...")}
  GET  /health, /readiness ("<pod> is healthy"/"... is ready"), /metrics

Sampling defaults follow the reference (temperature 0.7, top-k 50, top-p 0.9,
app/vllm_model_api.py:24; ``SHAI_TEMPERATURE`` overrides the temperature, 0 =
greedy).  Unlike vllm_model_api.py:38-43, ``max_new_tokens`` is honoured (the _m
variant's behaviour).  Engine kwargs come from a /vllm_config.yaml-style file
(``VLLM_CONFIG``): tensor_parallel_size, max_num_seqs, max_model_len, block_size
(rounded to 64-token KV blocks), quantization (``fp8``: e4m3 weights + per-row
scales, bf16 activations; ``mxfp4``: OCP MXFP4 weights -- e2m1 codes with one
e8m0 scale per 32 inputs, quantised on load -- bf16 activations: the 4-bit
deployment of the reference's bitsandbytes ``load_in_4bit`` models) and
kv_cache_dtype (``auto`` / ``bf16``, or ``fp8`` / ``fp8_e4m3``: OCP e4m3fn KV
cache with scalar k/v scales -- half the KV bytes per decode step, twice the
tokens per block pool; every TP rank reads the same file, so the relaunched
ranks build the same cache) with kv_prefill (``widen``, the default, or
``native``: the prefill attention reads the fp8 cache directly and the engine
holds no bf16 scratch) and speculative_config (vLLM's keys: ``method: ngram``,
``num_speculative_tokens`` 1..7, ``prompt_lookup_max`` 4, ``prompt_lookup_min``
1: pure decode steps verify n-gram drafts from the sequence's own tokens, up to
1 + k tokens per sequence and step; the responses do not change.  Off when
absent; text models only).

Tensor parallelism (``tensor_parallel_size: N``, app/vllm_model_api.py:127-129 with
cova/mllama-32-11b-vllm-trn1-config.yaml:9): the worker runs as N processes, one
per GPU (the supervisor launches ``torch.distributed.run --nproc-per-node N``; a
bare ``python -m ...llm_api`` relaunches itself that way).  Rank 0 serves HTTP and
broadcasts each engine step's new requests to the other ranks, which run the same
step (serving/tp.py).

``image``: with a Llama-3.2-Vision model (``MODEL_ID`` containing "vision", or a
local checkpoint with a ``vision_config``) the image goes through the native
vision tower and the decoder's cross-attention layers (models/mllama.py); a
text-only model validates and acknowledges it without attending to it.
"""

import base64
import io
import os
import time
import traceback
from typing import Dict, List, Optional

from .common import METRICS, LatencyCollector, ServerEnv, b64text, base_app, latency_report, mount_ui


def load_vllm_config(path: Optional[str]) -> dict:
    if not path or not os.path.exists(path):
        return {}
    import yaml
    with open(path) as f:
        return yaml.safe_load(f) or {}


def _vllm_config() -> dict:
    return load_vllm_config(os.environ.get("VLLM_CONFIG", "/vllm_config.yaml"))


def tp_degree(vc: dict) -> int:
    from .tp import env_tp_degree
    return int(vc.get("tensor_parallel_size") or env_tp_degree())


def build_engine(env: ServerEnv, vc: Optional[dict] = None):
    """The (TP-sharded, when the process group is up) engine; identical on every rank."""
    from ..engines.llm import LLMEngine, llama_config_for
    vc = _vllm_config() if vc is None else vc
    cfg = llama_config_for(env.model_id, env.model_path, env.config)
    text = getattr(cfg, "text", cfg)   # MllamaConfig (vision) or LlamaConfig
    eng = LLMEngine(cfg, device=env.torch_device, model_path=env.model_path,
                    max_num_seqs=int(vc.get("max_num_seqs", 64)),
                    max_model_len=int(vc.get("max_model_len", min(8192, text.max_position_embeddings))),
                    enable_prefix_caching=True, quantization=vc.get("quantization"),
                    kv_cache_dtype=vc.get("kv_cache_dtype"), kv_prefill=vc.get("kv_prefill"),
                    speculative=vc.get("speculative_config"))
    import torch
    with torch.inference_mode():
        # every decode batch bucket (sampled and all-greedy) captured before the first request
        eng.warmup_graphs(greedy_too=True)
    return eng


def build_service(env: ServerEnv, tpc=None):
    from ..engines.llm import LLMService
    from ..tokenizers import load_tokenizer
    eng = build_engine(env)
    cfg = eng.mcfg if eng.mcfg is not None else eng.cfg
    text = eng.cfg
    specials = {"<|begin_of_text|>": text.bos_token_id}
    if text is not cfg:
        specials["<|image|>"] = cfg.image_token_index
    tok = load_tokenizer(env.model_path, vocab_size=text.vocab_size, bos_id=text.bos_token_id,
                         eos_id=text.eos_token_id, pad_id=0, model_max_length=eng.max_model_len, specials=specials)
    channel = None
    if tpc is not None and tpc.enabled:
        tpc.start_heartbeat()
        channel = tpc.channel
    return LLMService(eng, tok, channel=channel)


def _decode_image(b64: str):
    from PIL import Image
    raw = base64.b64decode(b64.split(",", 1)[-1])
    return Image.open(io.BytesIO(raw)).convert("RGB")


def add_instruct(prompt: str, has_image: bool) -> str:
    """Llama-3 instruct turn around the user prompt, with the image placeholder first when an image is
    attached (the formatting app/vllm_model_api_m.py:47 applies through NxDI's ``add_instruct``)."""
    img = "<|image|>" if has_image else ""
    return (f"<|begin_of_text|><|start_header_id|>user<|end_header_id|>\n\n{img}{prompt}<|eot_id|>"
            f"<|start_header_id|>assistant<|end_header_id|>\n\n")


def create_app(service=None, env: Optional[ServerEnv] = None, tpc=None):
    from fastapi import HTTPException
    from pydantic import BaseModel, Field

    from ..engines.llm import SamplingParams
    env = env or ServerEnv.from_env(app="llm")
    service = service or build_service(env, tpc)
    temperature = float(os.environ.get("SHAI_TEMPERATURE", "0.7"))

    class GenerateRequest(BaseModel):
        max_new_tokens: int = 128
        prompt: str
        image: Optional[str] = None
        # vLLM's request-level sampling options; an absent field keeps the server's value (SHAI_TEMPERATURE, 50,
        # 0.9, no penalties); a value out of range is a 422
        temperature: Optional[float] = Field(None, ge=0.0)
        top_k: Optional[int] = None
        top_p: Optional[float] = Field(None, gt=0.0, le=1.0)
        min_p: Optional[float] = Field(None, ge=0.0, le=1.0)
        repetition_penalty: Optional[float] = Field(None, gt=0.0)
        presence_penalty: Optional[float] = Field(None, ge=-2.0, le=2.0)
        frequency_penalty: Optional[float] = Field(None, ge=-2.0, le=2.0)
        seed: Optional[int] = None
        logprobs: Optional[int] = Field(None, ge=0, le=20)
        # constraints (engines/constraints.py): OpenAI's logit_bias object, vLLM's allowed_token_ids / min_tokens /
        # bad_words / guided_choice; the string forms need the service's tokenizer, the *_ids forms do not
        logit_bias: Optional[Dict[str, float]] = None
        allowed_token_ids: Optional[List[int]] = None
        min_tokens: Optional[int] = Field(None, ge=0)
        bad_words: Optional[List[str]] = None
        bad_words_ids: Optional[List[List[int]]] = None
        guided_choice: Optional[List[str]] = None
        guided_choice_ids: Optional[List[List[int]]] = None

    SAMPLING_FIELDS = ("temperature", "top_k", "top_p", "min_p", "repetition_penalty", "presence_penalty",
                       "frequency_penalty", "seed", "logprobs")

    class GenerateBenchmarkRequest(BaseModel):
        n_runs: int
        max_new_tokens: int
        prompt: str

    class GenerateResponse(BaseModel):
        text: str = Field(..., description="Base64-encoded text")
        execution_time: float
        logprobs: Optional[list] = None   # one entry per generated token; present only when the request asked

    class GenerateBenchmarkResponse(BaseModel):
        report: str = Field(..., description="Benchmark report")

    def tokenise(text, what):
        tok = getattr(service, "tokenizer", None)
        if tok is None or not hasattr(tok, "encode"):
            raise HTTPException(status_code=422, detail=f"{what}: this service has no tokenizer, send {what}_ids")
        try:
            ids = tok.encode(text, add_special_tokens=False)
        except TypeError:
            ids = tok.encode(text)
        ids = [int(i) for i in ids]
        if not ids:
            raise HTTPException(status_code=422, detail=f"{what}: {text!r} tokenises to nothing")
        return ids

    def params(n, request=None):
        p = SamplingParams(temperature=temperature, top_k=50, top_p=0.9, max_tokens=max(1, int(n)))
        for name in SAMPLING_FIELDS if request is not None else ():
            v = getattr(request, name)
            if v is not None:
                setattr(p, name, v)
        if request is None:
            return p
        if request.logit_bias is not None:
            try:
                p.logit_bias = {int(k): float(v) for k, v in request.logit_bias.items()}
            except ValueError:
                raise HTTPException(status_code=422, detail="logit_bias keys must be token ids") from None
        if request.allowed_token_ids is not None:
            p.allowed_token_ids = list(request.allowed_token_ids)
        if request.min_tokens is not None:
            p.min_tokens = request.min_tokens
        for field, strings, ids in (("bad_words_ids", request.bad_words, request.bad_words_ids),
                                    ("guided_choice", request.guided_choice, request.guided_choice_ids)):
            if strings is not None or ids is not None:
                what = "bad_words" if field == "bad_words_ids" else "guided_choice"
                setattr(p, field, [list(w) for w in ids or ()] + [tokenise(t, what) for t in strings or ()])
        try:
            p.validate()
        except ValueError as e:
            raise HTTPException(status_code=422, detail=str(e)) from None
        return p

    multimodal = bool(getattr(service, "multimodal", False))

    def gentext(prompt: str, max_new_tokens: int, image_b64: Optional[str] = None, request=None):
        image = None
        if image_b64:
            image = _decode_image(image_b64)
            prompt = add_instruct(prompt, True)
            if not multimodal:
                image = None  # text-only model: the image is validated and acknowledged, not attended to
        p = params(max_new_tokens, request)
        try:
            text, secs, seq = service.generate_text(prompt, p, image=image)
        except ValueError as e:   # constraints that do not compile against the vocabulary (ids out of range, ...)
            if not p.constrained:
                raise
            raise HTTPException(status_code=422, detail=str(e)) from None
        if request is not None:
            return text, secs, seq
        return text, secs

    def bench(n_runs, test_name, prompt, max_new_tokens):
        gentext(prompt, max_new_tokens)  # warm-up run, as the reference
        lc = LatencyCollector()
        for _ in range(max(1, n_runs)):
            lc.pre_hook()
            gentext(prompt, max_new_tokens)
            lc.hook()
        return latency_report(lc, test_name)

    # import-time warm-up (vllm_model_api.py:131-133 runs benchmark(10, "warmup"))
    bench(2, "warmup", "What model are you?", 8)

    app = base_app(env, f"{env.model_id} LLM API", spaced=True)
    app.state.service = service

    @app.post("/benchmark", response_model=GenerateBenchmarkResponse)
    def generate_benchmark_report(request: GenerateBenchmarkRequest):
        try:
            test_name = f"benchmark:{env.app} on {env.nodepool} with {request.max_new_tokens} output tokens"
            report = bench(request.n_runs, test_name, request.prompt, request.max_new_tokens)
            return GenerateBenchmarkResponse(report=b64text(report))
        except Exception as e:
            traceback.print_exc()
            raise HTTPException(status_code=500, detail=f"{e}")

    @app.post("/generate", response_model=GenerateResponse, response_model_exclude_none=True)
    def generate_text_post(request: GenerateRequest):
        try:
            text, total, seq = gentext(request.prompt, request.max_new_tokens, request.image, request)
            METRICS.request_done(env, total)
            lps = list(seq.logprobs) if request.logprobs is not None else None
            return GenerateResponse(text=b64text(text), execution_time=total, logprobs=lps)
        except HTTPException:
            raise
        except Exception as e:
            traceback.print_exc()
            raise HTTPException(status_code=500, detail=f"text serialization failed: {e}")

    mount_ui(app, f"{env.model_id} on MI355X", "/generate", "{prompt: p, max_new_tokens: 64}")
    return app


def main():
    from . import tp as tp_serving
    from ..engines.llm import engine_step
    vc = _vllm_config()
    env = ServerEnv.from_env(app="llm")
    # follower ranks mirror rank 0's engine steps (each STEP message = the requests admitted since the last)
    tp_serving.serve("shai_amd.serving.llm_api", tp_degree(vc), lambda: build_engine(env, vc),
                     lambda tpc: create_app(env=env, tpc=tpc),
                     step_fn=lambda eng: (lambda adds: engine_step(eng, adds)))


if __name__ == "__main__":
    main()
