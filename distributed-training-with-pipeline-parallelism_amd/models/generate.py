"""Autoregressive generation with a KV cache for the pre-norm native models (GPT-2, Llama-3).

A :class:`Generator` holds the whole model as one single-stage :class:`NativeModel` and runs
it in two modes that share the training weights (the stage's :class:`ParamArena`) and ops:

* :meth:`Generator.prefill` -- the prompt through the training-path kernels (``attn_fwd``
  with ``Sq = Sk = S0``, causal), keeping every layer's K/V rows in a :class:`KVCache`;
* :meth:`Generator.decode` -- one new token per sequence: [B, D] rows through the same
  norm / GEMM / activation ops and :func:`ops.attn_decode` (csrc/kernels/
  attention_decode.hip: split-KV single-token attention over the cache).

Only the last position's rows reach the final norm and the LM head.  A decode step issues
no host synchronisation: the position is a host counter (prompts of a batch share one
length), the per-sequence ``lens`` the kernel reads live on the device.  On CPU tensors
everything runs through the ops' f32 reference paths.

Ragged batches (:meth:`Generator.generate_batch`, ``prefill(lens=)``): prompts of different
lengths are right-padded for the prefill, and the decode step then reads every position
from ``cache.lens`` on the device (csrc/kernels/generate.hip: position-aware embedding,
fused RoPE + K/V append at ``lens[b]``, on-device sampling with top-k / top-p and a stop
token).  That step takes no host value that changes from token to token, so it can be
captured once as a HIP graph and replayed (``graphs=True``).

Several tokens at once (:meth:`Generator.extend`): ``T`` new tokens per sequence are appended
at ``cache.lens[b] ...`` and attend causally over the cache plus the earlier new tokens
(csrc/kernels/attention_append.hip: MFMA attention with device-side lengths, split over the
keys).  That is a second prompt over an existing cache, a chunked prefill, the scoring of a
continuation, and the verification pass of greedy speculative decoding
(:meth:`Generator.generate_speculative`, with :meth:`KVCache.truncate` as the rollback).

int8 weight-only inference (``Generator(..., weights="int8")``, :class:`QuantWeights`): the
block matrices and the LM head are held as int8 with one f32 scale per output row and no
training state, and linear layers of at most 16 rows stream them through
csrc/kernels/gemv_skinny.hip (:func:`ops.linear_w8`); ``skinny=True`` runs bf16 weights
through the same kernel.  ``weights="int4g128"`` holds the same matrices as packed 4-bit
values with one f32 scale per 128-element group of K (:func:`ops.quantize_w4`,
:func:`ops.linear_w4`): half the streamed bytes again.  Every mode above works on every kind
of generator.  The formats are the entries of ``ops.QUANT_FORMATS`` (ops/quant.py); this module
reaches them only by name, through that table and :func:`ops.linear_q`.

int8 KV cache (``Generator(..., kv_cache="int8")``, ``KVCache(..., kv="int8")``): every K / V
row is stored as int8 with one f32 scale per (token, KV head) inside the row
(:func:`ops.generate.kv_quantize`; csrc/kernels/attention_kv8.hip), 0.52-0.53x the bytes of
bf16.  Every writer goes through the quantising :func:`ops.rope_kv_append`, the attention ops
read the rows as stored.  Independent of ``weights=`` and ``skinny=``.  A prefill attends to its
own exact K / V and stores them quantised; :meth:`Generator.extend` (also from an empty cache)
appends first and attends to the quantised rows, its own tokens' included, as every decode
step does.
"""
from __future__ import annotations

import dataclasses
from typing import Dict, List, Optional

import torch

from .. import ops
from .config import NativeConfig
from .native import Block, NativeModel, ParamSpec, _name_seed, block_param_specs


def _check_generative(cfg: NativeConfig) -> None:
    if cfg.cross_attn or not cfg.causal or not cfg.pre_norm:
        raise ValueError(f"{cfg.name}: generation needs a causal pre-norm decoder "
                         "(the reference post-LN cross-attention model is not a generator)")


KV_FORMATS = ("bf16", "int8")


def _check_kv(kv: str) -> str:
    if kv not in KV_FORMATS:
        raise ValueError(f"KV cache format must be one of {KV_FORMATS}, got {kv!r}")
    return kv


class KVCache:
    """Per-layer K / V rows ``[B, max_len, Hkv * Dh]`` (K after RoPE) plus the number of
    valid rows: ``lens`` (int32 [B], on the device, what the decode kernel reads) and
    ``pos`` (the same number on the host; the sequences of a batch advance together).

    ``kv="bf16"`` (the default) keeps the rows in ``dtype``; ``kv="int8"`` keeps them as int8
    ``[B, max_len, W]`` rows with their scales inside (``W = ops.generate.kv8_row_bytes(Hkv,
    Dh)``).  ``nbytes``: the bytes of all K / V rows of either kind."""

    def __init__(self, cfg: NativeConfig, B: int, max_len: int, device, dtype=torch.bfloat16, kv: str = "bf16"):
        if max_len < 1 or max_len > cfg.max_seq_len:
            raise ValueError(f"KVCache: max_len {max_len} outside [1, max_seq_len = {cfg.max_seq_len}]")
        self.kv = _check_kv(kv)
        self.B, self.max_len = int(B), int(max_len)
        self.device = torch.device(device)
        kv = cfg.n_kv_heads * cfg.head_dim
        if self.kv == "int8":
            kv, dtype = ops.generate.kv8_row_bytes(cfg.n_kv_heads, cfg.head_dim), torch.int8
        self.k: List[torch.Tensor] = [torch.zeros(B, max_len, kv, device=self.device, dtype=dtype)
                                      for _ in range(cfg.n_layers)]
        self.v: List[torch.Tensor] = [torch.zeros(B, max_len, kv, device=self.device, dtype=dtype)
                                      for _ in range(cfg.n_layers)]
        self.lens = torch.zeros(B, device=self.device, dtype=torch.int32)
        self.pos = 0
        # ragged: the sequences have their own lengths (prefill(lens=)): ``lens`` is then the
        # only record of a position, ``pos`` a host upper bound of max(lens), and ``positions``
        # (int32 [B], static so a captured step finds it) holds lens as it was when the
        # current decode step began -- where that step's token is embedded and appended
        self.ragged = False
        self.positions = torch.zeros(B, device=self.device, dtype=torch.int32)

    @property
    def nbytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in self.k + self.v)

    def reset(self) -> None:
        self.lens.zero_()
        self.pos = 0
        self.ragged = False

    def truncate(self, lens, pos: Optional[int] = None) -> None:
        """Roll the cache back to ``lens`` valid rows per sequence: a device tensor or host
        ints [B], each at most the current value (not checked for a device tensor: that would
        be a host synchronisation).  The cache becomes ragged.  ``pos`` is the new host upper
        bound of the lengths; by default ``max(lens)`` for host ints and the old bound for a
        device tensor.  Rows past ``lens[b]`` are stale, which every kernel tolerates."""
        if isinstance(lens, torch.Tensor) and lens.device.type != "cpu":
            if lens.numel() != self.B:
                raise ValueError(f"truncate: {lens.numel()} lengths for a cache of {self.B} sequences")
            self.lens.copy_(lens.reshape(-1))
            bound = self.pos if pos is None else int(pos)
        else:
            host = torch.as_tensor(lens).reshape(-1).to(torch.int64)
            if host.numel() != self.B or int(host.min()) < 0 or int(host.max()) > self.pos:
                raise ValueError(f"truncate: needs {self.B} lengths in [0, {self.pos}]")
            self.lens.copy_(host)
            bound = int(host.max()) if pos is None else int(pos)
        if bound < 0 or bound > self.max_len:
            raise ValueError(f"truncate: pos {bound} outside [0, {self.max_len}]")
        self.pos = bound
        self.ragged = True


QUANTIZED = ("attn.wqkv.weight", "attn.wo.weight", "ffn.w1.weight", "ffn.w2.weight", "ffn.w13.weight")
QUANT_FORMATS = tuple(ops.QUANT_FORMATS)


def model_param_specs(cfg: NativeConfig) -> List[ParamSpec]:
    """The parameters of a whole single-stage generative model, by the FQNs a
    :class:`NativeModel` at ``pp = 1`` (and a checkpoint) gives them."""
    d = cfg.d_model
    specs = [ParamSpec("tok_embeddings.weight", (cfg.vocab_padded, d), "normal", False, cfg.init_std)]
    if cfg.pos == "learned":
        specs.append(ParamSpec("pos_embeddings.weight", (cfg.max_seq_len, d), "normal", False, 0.01))
    for i in range(cfg.n_layers):
        specs += block_param_specs(cfg, i)
    if cfg.final_norm:
        specs.append(ParamSpec("norm.weight", (d,), "ones", False))
        if cfg.norm == "layernorm":
            specs.append(ParamSpec("norm.bias", (d,), "zeros", False))
    if not cfg.tie_embeddings:
        specs.append(ParamSpec("output.weight", (cfg.vocab_padded, d), "normal", True, cfg.init_std))
    return specs


class QuantWeights:
    """Inference-only weights of a whole model with its matrices in int8: what a quantised
    :class:`Generator` holds instead of a :class:`ParamArena`.

    Every block matrix (``QUANTIZED``) and the LM head are kept as ``q[name]`` (int8 [N, K])
    and ``scale[name]`` (f32 [N]), the format of :func:`ops.quantize_w8`; embeddings, norms and
    biases as ``dtype`` tensors.  With tied embeddings the head is an int8 copy of the token
    table (``q["tok_embeddings.weight"]``) beside the table itself.  There is no f32 master, no
    gradient, no transposed copy and no dense copy of a quantised matrix.  ``w`` / ``has``
    answer as the arena does for the dense tensors.

    ``fmt="int4g128"``: ``q[name]`` is packed uint8 [N, K / 2] and ``scale[name]`` f32
    [K / 128, N], the format of :func:`ops.quantize_w4`; every quantised matrix needs
    ``K % 128 == 0`` (checked here, before anything is stored)."""

    def __init__(self, cfg: NativeConfig, device, dtype=torch.bfloat16, fmt: str = "int8"):
        if fmt not in QUANT_FORMATS:
            raise ValueError(f"QuantWeights: format must be one of {QUANT_FORMATS}, got {fmt!r}")
        self.fmt = fmt
        self.cfg = cfg
        self.device = torch.device(device)
        self.dtype = dtype
        specs = model_param_specs(cfg)
        self.specs = {s.name: s for s in specs}
        self.order = [s.name for s in specs]
        self.head_name = "tok_embeddings.weight" if cfg.tie_embeddings else "output.weight"
        self.q: Dict[str, torch.Tensor] = {}
        self.scale: Dict[str, torch.Tensor] = {}
        self.dense: Dict[str, torch.Tensor] = {}
        mult = ops.QUANT_FORMATS[fmt].k_format
        bad = [(n, self.specs[n].shape) for n in self.order if self.quantized(n) and self.specs[n].shape[1] % mult != 0]
        if bad:
            raise ValueError(f"QuantWeights: {fmt} needs K % {mult} == 0 in every quantised matrix; "
                             f"{bad[0][0]} is {tuple(bad[0][1])}")

    def quantized(self, name: str) -> bool:
        return name == self.head_name or name.endswith(QUANTIZED)

    def has(self, name: str) -> bool:
        return name in self.specs

    def w(self, name: str) -> torch.Tensor:
        return self.dense[name]

    def put(self, name: str, t: torch.Tensor) -> None:
        """Store one parameter from its full-precision values: quantised on the target
        device where the name calls for it, cast to ``dtype`` otherwise."""
        # quantised where the values are (a checkpoint's tensors on the host: the device then
        # sees only the int8 matrix, never an f32 temporary whose freed block a later tensor
        # would take over whole); quantize_w8 gives the same values on either device
        s = self.specs[name]
        t = t.detach().float().reshape(s.shape)
        if self.quantized(name):
            q, scale = ops.QUANT_FORMATS[self.fmt].quantize(t)
            self.q[name], self.scale[name] = q.to(self.device), scale.to(self.device)
        # dense: everything but the block matrices and an untied head (a tied head is also
        # the embedding table, which stays dense)
        if not name.endswith(QUANTIZED) and (name != self.head_name or self.cfg.tie_embeddings):
            self.dense[name] = t.to(self.dtype, copy=True).contiguous().to(self.device)     # never a view of the source

    def init_params(self, seed: int = 0) -> None:
        """The values :meth:`ParamArena.init_params` draws for the same seed, quantised."""
        gdev = "cuda" if self.device.type == "cuda" else "cpu"
        for name in self.order:
            s = self.specs[name]
            if s.init == "zeros":
                v = torch.zeros(s.shape)
            elif s.init == "ones":
                v = torch.ones(s.shape)
            else:
                g = torch.Generator(device=gdev).manual_seed(_name_seed(seed, name))
                v = torch.randn(s.shape, generator=g, device=gdev, dtype=torch.float32) * s.std
            self.put(name, v)

    def load_state_dict(self, sd: Dict[str, torch.Tensor]) -> None:
        missing = [n for n in self.order if n not in sd]
        if missing:
            raise KeyError(f"missing keys: {missing[:5]}...")
        for n in self.order:
            self.put(n, sd[n])

    def _what(self, n: str) -> torch.Tensor:
        return ops.QUANT_FORMATS[self.fmt].dequant(self.q[n].cpu(), self.scale[n].cpu())

    def effective_state_dict(self) -> Dict[str, torch.Tensor]:
        """f32 CPU tensors by FQN of the weights this generator computes with: ``q * scale``
        (per row, or per group of 128 k for int4g128) for the quantised matrices (also for
        the head of an untied model), the stored values otherwise.  With tied embeddings ``tok_embeddings.weight`` is the embedding table and
        the head's effective weight is under ``"lm_head"``."""
        out = {}
        for n in self.order:
            if n in self.dense:
                out[n] = self.dense[n].detach().float().cpu()
            else:
                out[n] = self._what(n)
        if self.cfg.tie_embeddings:
            out["lm_head"] = self._what(self.head_name)
        return out

    def max_matrix_numel(self) -> int:
        """N * K of the largest quantised matrix: what the dequantisation scratch must hold (a
        packed 4-bit tensor has half as many elements)"""
        return max(self.specs[n].shape[0] * self.specs[n].shape[1] for n in self.q)


class _QBlock:
    """What the generator reads of a :class:`Block`, over :class:`QuantWeights`."""

    def __init__(self, idx: int, weights: QuantWeights, rope=None):
        self.i = idx
        self.A = weights
        self.P = f"layers.{idx}."
        self.rope = rope

    def w(self, n):
        return self.A.w(self.P + n)

    def wb(self, n):
        return self.A.w(self.P + n) if self.A.has(self.P + n) else None


def _check_weights(weights: str, skinny: bool) -> None:
    if weights != "bf16" and weights not in QUANT_FORMATS:
        raise ValueError(f"Generator: weights must be 'bf16', 'int8' or 'int4g128', got {weights!r}")
    if skinny and weights != "bf16":
        raise ValueError("Generator: skinny=True is the bf16 weights' opt-in (quantised weights always use the skinny "
                         "kernel)")


class Generator:
    """KV-cache inference over one whole-model :class:`NativeModel` (``recompute=False``,
    dropout off: the training forward hands ``cfg.dropout`` to its kernels).

    ``weights="int8"``: the block matrices and the LM head are quantised per output row
    (:func:`ops.quantize_w8`) and the generator holds :class:`QuantWeights` instead of a model
    and its arena (``self.model`` is None).  Linear layers of at most ``ops.W8_SKINNY_MAX_M``
    rows read the int8 matrix directly (:func:`ops.linear_skinny`); larger ones (a prefill)
    dequantise into one scratch matrix, allocated on the first call that needs it.  GELU /
    SwiGLU models only.  ``weights="int4g128"``: the same with 4-bit values and one scale per
    128-element group of K (:func:`ops.quantize_w4`, :func:`ops.linear_w4`); every quantised
    matrix then needs ``K % 128 == 0``.  ``skinny=True`` (bf16 weights on the GPU only): linear layers of at
    most 16 rows run the bf16 instantiation of the same kernel instead of the training GEMM.

    ``kv_cache="int8"``: the caches :meth:`new_cache` makes (and so those of the ``generate*``
    methods) hold int8 rows (:class:`KVCache`); any kind of weights."""

    def __init__(self, cfg: NativeConfig, device, dtype=torch.bfloat16, seed: int = 0, init: bool = True,
                 weights: str = "bf16", skinny: bool = False, kv_cache: str = "bf16"):
        _check_generative(cfg)
        _check_weights(weights, skinny)
        self.kv_cache = _check_kv(kv_cache)
        cfg = dataclasses.replace(cfg, dropout=0.0)
        if weights != "bf16":
            qw = QuantWeights(cfg, device, dtype, weights)
            if init:
                qw.init_params(seed)
            self._bind_quant(qw)
            return
        self._bind(NativeModel(cfg, 0, 1, torch.device(device), seed=seed, recompute=False, dtype=dtype, init=init))
        self.skinny = bool(skinny)

    def _bind(self, model: NativeModel) -> None:
        self.model = model
        self.cfg = dataclasses.replace(model.cfg, dropout=0.0)
        self.arena = model.arena
        self.device = model.device
        self.dtype = model.arena.dtype
        self.blocks: List[Block] = model.blocks
        self.weights = "bf16"
        self.skinny = False
        self._scratch = None

    def _bind_quant(self, qw: QuantWeights) -> None:
        cfg = qw.cfg
        self.model = None
        self.cfg = cfg
        self.arena = qw
        self.device = qw.device
        self.dtype = qw.dtype
        rope = None
        if cfg.pos == "rope":
            rope = ops.rope_tables(cfg.max_seq_len, cfg.head_dim, cfg.rope_theta, self.device)
        self.blocks = [_QBlock(i, qw, rope) for i in range(cfg.n_layers)]
        self.weights = qw.fmt
        self.skinny = False
        self._scratch: Optional[torch.Tensor] = None

    # ------------------------------------------------------------------ constructors
    @classmethod
    def from_model(cls, model: NativeModel, weights: str = "bf16", skinny: bool = False,
                   kv_cache: str = "bf16") -> "Generator":
        """Wrap an existing single-stage model (``trainer.stages[0].model`` at ``pp = 1``).
        With bf16 weights they are the model's arena itself: nothing is copied, and a later
        optimizer step is seen by the generator.  ``weights="int8"`` / ``"int4g128"`` take a quantised
        snapshot of the master weights instead: the model is left untouched, and the
        generator does NOT see later optimizer steps (build a new one after training on)."""
        _check_generative(model.cfg)
        _check_weights(weights, skinny)
        if model.num_stages != 1 or model.split_head:
            raise ValueError("Generator.from_model needs a single-stage model that owns its LM head (pp = 1)")
        self = cls.__new__(cls)
        self.kv_cache = _check_kv(kv_cache)
        if weights != "bf16":
            qw = QuantWeights(dataclasses.replace(model.cfg, dropout=0.0), model.device, model.arena.dtype, weights)
            with model.arena.unsharded():
                for n in qw.order:
                    qw.put(n, model.arena.master_view(n))
            self._bind_quant(qw)
            return self
        self._bind(model)
        self.skinny = bool(skinny)
        return self

    @classmethod
    def load(cls, path: str, device=None, dtype=None, weights: str = "bf16", skinny: bool = False,
             kv_cache: str = "bf16") -> "Generator":
        """Weights-only load of a checkpoint directory written by ``save_checkpoint`` at any
        PP / DP degree or head mode (the tensors are found by FQN).  Defaults: the GPU in
        bf16 when there is one, else the CPU in f32.  ``weights="int8"`` / ``"int4g128"`` quantise
        tensor by tensor while loading (deterministic: the same checkpoint gives the same values)."""
        from ..utils.checkpoint import iter_weights, load_weights, read_manifest
        man = read_manifest(path)
        cfg = NativeConfig(**man["model"])
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else "cpu"
        device = torch.device(device)
        if dtype is None:
            dtype = torch.bfloat16 if device.type == "cuda" else torch.float32
        self = cls(cfg, device, dtype=dtype, init=False, weights=weights, skinny=skinny, kv_cache=kv_cache)
        if weights != "bf16":
            for name, t in iter_weights(path, self.arena.order):
                self.arena.put(name, t)
            return self
        load_weights([self.arena], path, strict=True)
        return self

    # ------------------------------------------------------------------ linear layers
    def _linear(self, x: torch.Tensor, wname: str, bname: Optional[str] = None, act: str = "none",
                residual: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        A = self.arena
        bias = A.w(bname) if bname is not None and A.has(bname) else None
        if self.weights != "bf16":
            key = A.head_name if wname == "lm_head" else wname
            q, scale = A.q[key], A.scale[key]
            scratch, kmult = None, ops.QUANT_FORMATS[self.weights].k_skinny
            if x.is_cuda and (x.shape[0] > ops.W8_SKINNY_MAX_M or x.shape[1] % kmult != 0):
                if self._scratch is None:
                    if torch.cuda.is_current_stream_capturing():
                        raise RuntimeError("Generator: the dequantisation scratch cannot be allocated inside a graph "
                                           "capture (run one step eagerly first)")
                    self._scratch = torch.empty(A.max_matrix_numel(), device=self.device, dtype=torch.bfloat16)
                scratch = self._scratch
            return ops.linear_q(x, q, scale, self.weights, bias, act, residual, out, scratch=scratch)
        w = self.model.head_weight() if wname == "lm_head" else A.w(wname)
        if self.skinny and x.is_cuda and x.dtype == torch.bfloat16 and x.shape[0] <= ops.SKINNY_MAX_M \
                and w.shape[1] % 32 == 0 and act in ("none", "gelu", "gelu_tanh"):
            return ops.linear_skinny(x, w, None, bias, act, residual, out)
        return ops.linear(x, w, bias, act=act, residual=residual, out=out)[0]

    # ------------------------------------------------------------------ cache
    def new_cache(self, B: int, max_len: Optional[int] = None, kv: Optional[str] = None) -> KVCache:
        """``kv``: "bf16" / "int8"; None = the generator's ``kv_cache``."""
        return KVCache(self.cfg, B, self.cfg.max_seq_len if max_len is None else max_len, self.device, self.dtype,
                       kv=self.kv_cache if kv is None else kv)

    # ------------------------------------------------------------------ layers
    def _norm(self, x, w, b):
        return ops.norm_fwd(x, w, b, kind=self.cfg.norm, eps=self.cfg.norm_eps)[0]

    def _ffn(self, blk: Block, x2: torch.Tensor) -> torch.Tensor:
        cfg = self.cfg
        h2 = self._norm(x2, blk.w("ffn_norm.weight"), blk.wb("ffn_norm.bias"))
        if cfg.activation == "swiglu":
            gu = self._linear(h2, blk.P + "ffn.w13.weight")
            return self._linear(ops.swiglu_fwd(gu), blk.P + "ffn.w2.weight", residual=x2)
        g = self._linear(h2, blk.P + "ffn.w1.weight", blk.P + "ffn.w1.bias", act=cfg.activation)
        return self._linear(g, blk.P + "ffn.w2.weight", blk.P + "ffn.w2.bias", residual=x2)

    def _qkv(self, blk: Block, x: torch.Tensor, S: int, pos: int) -> torch.Tensor:
        cfg = self.cfg
        h1 = self._norm(x, blk.w("attn_norm.weight"), blk.wb("attn_norm.bias"))
        qkv = self._linear(h1, blk.P + "attn.wqkv.weight", blk.P + "attn.wqkv.bias")
        if cfg.pos == "rope":
            ops.rope_(qkv, blk.rope[0], blk.rope[1], S, cfg.n_heads, cfg.n_kv_heads, cfg.head_dim, pos_offset=pos)
        return qkv

    def _head(self, h: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Final norm + LM head of [B, D] rows -> logits [B, vocab_padded]."""
        A = self.arena
        if self.cfg.final_norm:
            h = self._norm(h, A.w("norm.weight"), A.w("norm.bias") if A.has("norm.bias") else None)
        return self._linear(h, "lm_head", "output.bias", out=out)

    def _embed(self, tokens: torch.Tensor, S: int, pos: int) -> torch.Tensor:
        A = self.arena
        return ops.embed_fwd(tokens.reshape(-1), A.w("tok_embeddings.weight"),
                             A.w("pos_embeddings.weight") if self.cfg.pos == "learned" else None, S, pos_offset=pos)

    # ------------------------------------------------------------------ the two modes
    @torch.no_grad()
    def prefill(self, tokens: torch.Tensor, cache: KVCache, lens=None) -> torch.Tensor:
        """tokens [B, S0] -> logits [B, vocab_padded] of the last position; fills ``cache``
        rows [0, S0) of every layer.

        With ``lens`` (host ints [B], ``1 <= lens[b] <= S0``) ``tokens`` is right-padded: row
        b holds ``lens[b]`` tokens, then anything.  Attention is causal, so padding never
        reaches an earlier position and the same kernels run; the logits are those of
        position ``lens[b] - 1``.  The cache becomes ragged: ``cache.lens = lens``, cache
        rows at and beyond ``lens[b]`` are stale (no decode step reads them), ``cache.pos``
        is only a host upper bound of the lengths."""
        cfg = self.cfg
        B, S = tokens.shape
        if B != cache.B or S < 1 or S > cache.max_len:
            raise ValueError(f"prefill: tokens {tuple(tokens.shape)} do not fit a cache of {cache.B} x {cache.max_len}")
        if lens is not None:
            lens = torch.as_tensor(lens).reshape(-1).to("cpu", torch.int64)
            if lens.numel() != B or int(lens.min()) < 1 or int(lens.max()) > S:
                raise ValueError(f"prefill: lens must hold {B} lengths in [1, {S}]")
        H, KV, Dh = cfg.n_heads, cfg.n_kv_heads, cfg.head_dim
        x = self._embed(tokens.to(self.device), S, 0)
        zero = torch.zeros(B, device=self.device, dtype=torch.int32) if cache.kv == "int8" else None
        for li, blk in enumerate(self.blocks):
            qkv = self._qkv(blk, x, S, 0)
            q, k, v = qkv[:, : H * Dh], qkv[:, H * Dh:(H + KV) * Dh], qkv[:, (H + KV) * Dh:]
            if cache.kv == "int8":
                # the rotated rows, quantised at positions 0 .. S - 1; attn_fwd below reads the exact ones
                ops.rope_kv_append(qkv, None, None, cache.k[li], cache.v[li], zero, None, H, KV, Dh, rope=False, T=S)
            else:
                cache.k[li][:, :S].copy_(k.view(B, S, KV * Dh))     # after RoPE: rope_ is in place
                cache.v[li][:, :S].copy_(v.view(B, S, KV * Dh))
            o = torch.empty(B * S, H * Dh, device=x.device, dtype=x.dtype)
            lse = torch.empty(B * H * S, device=x.device, dtype=torch.float32)
            ops.attn_fwd(q, k, v, o, lse, B, S, S, H, KV, Dh, True, p_drop=0.0)
            x2 = self._linear(o, blk.P + "attn.wo.weight", blk.P + "attn.wo.bias", residual=x)
            x = self._ffn(blk, x2)
        cache.pos = S
        if lens is None:
            cache.lens.fill_(S)
            cache.ragged = False
            return self._head(x.view(B, S, -1)[:, -1].contiguous())
        cache.lens.copy_(lens)
        cache.ragged = True
        last = torch.arange(B, device=x.device) * S + (lens.to(x.device) - 1)
        return self._head(x.index_select(0, last))

    def _decode_ragged(self, tokens: torch.Tensor, cache: KVCache, active: Optional[torch.Tensor],
                       out: Optional[torch.Tensor]) -> torch.Tensor:
        """The decode step of a ragged cache: every position is read from ``cache.lens`` on
        the device, so the launches and their arguments are the same at every token (the step
        can be captured once and replayed).  ``attn_decode`` runs over ``cache.max_len`` keys'
        worth of workgroups every step; rows past ``lens[b]`` never enter the result."""
        cfg = self.cfg
        B = cache.B
        H, KV, Dh = cfg.n_heads, cfg.n_kv_heads, cfg.head_dim
        if active is not None and (active.dtype != torch.uint8 or active.numel() != B or active.device != cache.lens.device):
            raise ValueError("decode: active must be uint8 [B] on the cache's device")
        cache.positions.copy_(cache.lens)          # where this token goes
        cache.lens.add_(1 if active is None else active)      # ... and it is a key too
        A = self.arena
        x = ops.embed_fwd(tokens.reshape(-1), A.w("tok_embeddings.weight"),
                          A.w("pos_embeddings.weight") if cfg.pos == "learned" else None, 1,
                          positions=cache.positions)
        rope = cfg.pos == "rope"
        for li, blk in enumerate(self.blocks):
            h1 = self._norm(x, blk.w("attn_norm.weight"), blk.wb("attn_norm.bias"))
            qkv = self._linear(h1, blk.P + "attn.wqkv.weight", blk.P + "attn.wqkv.bias")
            ops.rope_kv_append(qkv, blk.rope[0] if rope else None, blk.rope[1] if rope else None, cache.k[li],
                               cache.v[li], cache.positions, active, H, KV, Dh, rope=rope)
            o = torch.empty(B, H * Dh, device=x.device, dtype=x.dtype)
            ops.attn_decode(qkv[:, : H * Dh], cache.k[li], cache.v[li], cache.lens, o, H, KV, Dh,
                            max_len=cache.max_len)
            x2 = self._linear(o, blk.P + "attn.wo.weight", blk.P + "attn.wo.bias", residual=x)
            x = self._ffn(blk, x2)
        cache.pos += 1
        return self._head(x, out=out)

    @torch.no_grad()
    def decode(self, tokens: torch.Tensor, cache: KVCache, active: Optional[torch.Tensor] = None,
               out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """tokens [B] (the token at position ``cache.pos`` of every sequence) -> logits
        [B, vocab_padded] for the next position; appends one K/V row per layer.

        On a ragged cache (``prefill(lens=)``) row b's token goes to position ``lens[b]``.
        ``active`` (uint8 [B] on the device, ragged caches only): a row with ``active[b] ==
        0`` keeps its cache rows and its ``lens`` entry, and its logits row is unspecified.
        ``out``: a [B, vocab_padded] buffer for the logits."""
        cfg = self.cfg
        B, pos = cache.B, cache.pos
        if tokens.numel() != B:
            raise ValueError(f"decode: {tokens.numel()} tokens for a cache of {B} sequences")
        if pos < 1:
            raise ValueError("decode: prefill the cache first")
        if pos >= cache.max_len:
            raise ValueError(f"decode: the cache is full ({cache.max_len} positions)")
        if cache.ragged:
            return self._decode_ragged(tokens.to(self.device), cache, active, out)
        if active is not None:
            raise ValueError("decode: active needs a ragged cache (prefill(lens=...))")
        H, KV, Dh = cfg.n_heads, cfg.n_kv_heads, cfg.head_dim
        if cache.kv == "int8":
            cache.positions.copy_(cache.lens)      # = pos in every row: where the quantising append writes
        cache.lens.add_(1)            # the current token is a key too
        x = self._embed(tokens.to(self.device), 1, pos)
        for li, blk in enumerate(self.blocks):
            qkv = self._qkv(blk, x, 1, pos)
            q, k, v = qkv[:, : H * Dh], qkv[:, H * Dh:(H + KV) * Dh], qkv[:, (H + KV) * Dh:]
            if cache.kv == "int8":
                ops.rope_kv_append(qkv, None, None, cache.k[li], cache.v[li], cache.positions, None, H, KV, Dh,
                                   rope=False)
            else:
                cache.k[li][:, pos].copy_(k)
                cache.v[li][:, pos].copy_(v)
            o = torch.empty(B, H * Dh, device=x.device, dtype=x.dtype)
            ops.attn_decode(q, cache.k[li], cache.v[li], cache.lens, o, H, KV, Dh, max_len=pos + 1)
            x2 = self._linear(o, blk.P + "attn.wo.weight", blk.P + "attn.wo.bias", residual=x)
            x = self._ffn(blk, x2)
        cache.pos = pos + 1
        return self._head(x, out=out)

    @torch.no_grad()
    def extend(self, tokens: torch.Tensor, cache: KVCache, counts=None, all_logits: bool = False) -> torch.Tensor:
        """tokens [B, T]: append row b's first ``counts[b]`` tokens (host ints in [0, T];
        None = all T) at positions ``cache.lens[b] ...`` and return the logits
        [B, vocab_padded] of each row's last appended token, or [B, T, vocab_padded] of every
        position with ``all_logits=True`` (rows ``t >= counts[b]``, and the single row of a
        sequence with ``counts[b] == 0``, are unspecified but finite).

        Works on an empty cache (a prefill), a uniform and a ragged one.  Every position is
        read from ``cache.lens`` on the device; the host only checks ``cache.pos + T <=
        cache.max_len`` and advances ``cache.pos`` by T.  A row with ``counts[b] == 0`` keeps
        its cache rows and its length.  The cache becomes ragged unless it was uniform and
        ``counts`` is None.  All B * T rows go through the norm / GEMM / activation ops and
        :func:`ops.attn_append`; only the requested rows reach the LM head."""
        cfg = self.cfg
        if tokens.dim() != 2 or tokens.shape[0] != cache.B or tokens.shape[1] < 1:
            raise ValueError(f"extend: tokens {tuple(tokens.shape)} do not fit a cache of {cache.B} sequences")
        B, T = tokens.shape
        if cache.pos + T > cache.max_len:
            raise ValueError(f"extend: {cache.pos} cached + {T} new positions exceed the cache ({cache.max_len})")
        dev = self.device
        cnt = None
        if counts is not None:
            host = torch.as_tensor(counts).reshape(-1).to("cpu", torch.int64)
            if host.numel() != B or int(host.min()) < 0 or int(host.max()) > T:
                raise ValueError(f"extend: counts must hold {B} values in [0, {T}]")
            cnt = host.to(dev, torch.int32)
        H, KV, Dh = cfg.n_heads, cfg.n_kv_heads, cfg.head_dim
        A = self.arena
        base = cache.lens.clone()                    # the valid rows before this call
        positions = (base[:, None] + torch.arange(T, device=dev, dtype=torch.int32)[None, :]).reshape(-1)
        x = ops.embed_fwd(tokens.to(dev).reshape(-1), A.w("tok_embeddings.weight"),
                          A.w("pos_embeddings.weight") if cfg.pos == "learned" else None, 1, positions=positions)
        rope = cfg.pos == "rope"
        for li, blk in enumerate(self.blocks):
            h1 = self._norm(x, blk.w("attn_norm.weight"), blk.wb("attn_norm.bias"))
            qkv = self._linear(h1, blk.P + "attn.wqkv.weight", blk.P + "attn.wqkv.bias")
            ops.rope_kv_append(qkv, blk.rope[0] if rope else None, blk.rope[1] if rope else None, cache.k[li],
                               cache.v[li], base, None, H, KV, Dh, rope=rope, T=T, counts=cnt)
            o = torch.empty(B * T, H * Dh, device=x.device, dtype=x.dtype)
            ops.attn_append(qkv[:, : H * Dh], cache.k[li], cache.v[li], base, cnt, o, T, H, KV, Dh,
                            max_len=cache.pos + T)
            x2 = self._linear(o, blk.P + "attn.wo.weight", blk.P + "attn.wo.bias", residual=x)
            x = self._ffn(blk, x2)
        cache.lens.add_(T if cnt is None else cnt)
        cache.pos += T
        if cnt is not None:
            cache.ragged = True
        if all_logits:
            return self._head(x).view(B, T, -1)
        if cnt is None:
            return self._head(x.view(B, T, -1)[:, -1].contiguous())
        last = torch.arange(B, device=dev) * T + (cnt.long() - 1).clamp_(min=0)
        return self._head(x.index_select(0, last))

    # ------------------------------------------------------------------ sampling loop
    def _pick(self, logits: torch.Tensor, temperature: float, top_k: Optional[int],
              gen: Optional[torch.Generator]) -> torch.Tensor:
        lg = logits[:, : self.cfg.vocab_size].float()      # padded vocabulary columns are never emitted
        if temperature == 0:
            return lg.argmax(-1)
        lg = lg / temperature
        if top_k is not None and 0 < top_k < lg.shape[-1]:
            kth = lg.topk(int(top_k), dim=-1).values[:, -1:]
            lg = lg.masked_fill(lg < kth, float("-inf"))
        return torch.multinomial(torch.softmax(lg, -1), 1, generator=gen)[:, 0]

    @torch.no_grad()
    def generate(self, prompt: torch.Tensor, max_new_tokens: int, temperature: float = 0.0,
                 top_k: Optional[int] = None, seed: int = 0) -> torch.Tensor:
        """prompt [B, S0] (one shared length) -> [B, S0 + max_new_tokens] token ids.  Greedy
        at ``temperature == 0``; otherwise softmax sampling over the real vocabulary,
        optionally restricted to the ``top_k`` logits, from a generator seeded with ``seed``."""
        if prompt.dim() != 2 or prompt.shape[1] < 1:
            raise ValueError("generate: prompt must be [B, S0] with S0 >= 1")
        if temperature < 0 or max_new_tokens < 0:
            raise ValueError("generate: temperature and max_new_tokens must be >= 0")
        B, S0 = prompt.shape
        N = int(max_new_tokens)
        if S0 + N > self.cfg.max_seq_len:
            raise ValueError(f"generate: {S0} prompt + {N} new tokens exceed max_seq_len = {self.cfg.max_seq_len} "
                             "(the learned positions / RoPE table end there)")
        prompt = prompt.to(self.device, torch.int64)
        if N == 0:
            return prompt.clone()
        gen = None
        if temperature > 0:
            gen = torch.Generator(device=self.device).manual_seed(int(seed))
        out = torch.empty(B, S0 + N, device=self.device, dtype=torch.int64)
        out[:, :S0] = prompt
        cache = self.new_cache(B, S0 + N)
        logits = self.prefill(prompt, cache)
        for i in range(N):
            nxt = self._pick(logits, temperature, top_k, gen)
            out[:, S0 + i] = nxt
            if i + 1 < N:
                logits = self.decode(nxt, cache)
        return out

    @torch.no_grad()
    def generate_batch(self, prompts, max_new_tokens: int, temperature: float = 0.0, top_k: Optional[int] = None,
                       top_p: Optional[float] = None, seed: int = 0, stop_token: Optional[int] = None,
                       pad_token: int = 0, graphs: Optional[bool] = None):
        """Prompts of any lengths -> ``(out, lengths)``.

        ``prompts``: a list of 1-D int64 tensors (or lists of ids), each of length >= 1 with
        ``len + max_new_tokens <= max_seq_len``.  ``out`` is ``[B, max(len) + max_new_tokens]``:
        row b holds its prompt, then its new tokens up to and including ``stop_token``, then
        ``pad_token``; ``lengths[b]`` (int64, on the device) counts the valid tokens.

        Tokens are picked by :func:`ops.sample` (greedy at ``temperature == 0``, else
        temperature / ``top_k`` / ``top_p`` sampling) from ``u = torch.rand(N, B)`` of a
        generator seeded with ``seed``, drawn once up front: the same seed gives the same
        tokens with or without graphs.  One step -- sample, record, decode -- takes no host
        value that changes from token to token.  With ``graphs=True`` (GPU only; ``None``
        resolves to off: measured on the MI355X, replay is not faster than the eager step at
        B = 1 and within 1 % of it on all but one larger shape --
        profiles/r10_generate_batch.md) the first
        step runs eagerly, the second is captured as one HIP graph
        (parallel/graphs.py; every allocation of the step, ``attn_decode``'s workspace
        included, is made on the capturing stream and so comes from the graph's private pool)
        and the rest are replays.  No host synchronisation per token: without a stop token
        none at all, with one ``done.all()`` is read every 16th step to stop early."""
        cfg = self.cfg
        V, N, dev = cfg.vocab_size, int(max_new_tokens), self.device
        rows = [torch.as_tensor(p).reshape(-1).to("cpu", torch.int64) for p in prompts]
        if not rows or any(r.numel() < 1 for r in rows):
            raise ValueError("generate_batch: needs at least one prompt, each of at least one token")
        if temperature < 0 or N < 0:
            raise ValueError("generate_batch: temperature and max_new_tokens must be >= 0")
        lens = [int(r.numel()) for r in rows]
        B, S0 = len(rows), max(lens)
        if S0 + N > cfg.max_seq_len:
            raise ValueError(f"generate_batch: {S0} prompt + {N} new tokens exceed max_seq_len = {cfg.max_seq_len} "
                             "(the learned positions / RoPE table end there)")
        if any(int(r.min()) < 0 or int(r.max()) >= V for r in rows):
            raise ValueError(f"generate_batch: prompt token outside the vocabulary [0, {V})")
        pad, stop = int(pad_token), -1 if stop_token is None else int(stop_token)
        if not 0 <= pad < V:
            raise ValueError(f"generate_batch: pad_token {pad} outside the vocabulary [0, {V})")
        if stop_token is not None and not 0 <= stop < V:
            raise ValueError(f"generate_batch: stop_token {stop} outside the vocabulary [0, {V})")
        k = int(top_k or 0)
        p = 1.0 if top_p is None else float(top_p)
        if k < 0 or not 0.0 < p <= 1.0:
            raise ValueError("generate_batch: needs top_k >= 0 and 0 < top_p <= 1")
        use_graphs = False if graphs is None else bool(graphs)
        if use_graphs and dev.type != "cuda":
            raise ValueError("generate_batch: graphs need a GPU")

        tokens = torch.full((B, S0), pad, dtype=torch.int64)
        for b, r in enumerate(rows):
            tokens[b, : lens[b]] = r
        tokens = tokens.to(dev)
        out = torch.full((B, S0 + N), pad, device=dev, dtype=torch.int64)
        out[:, :S0] = tokens
        wpos = torch.tensor(lens, device=dev, dtype=torch.int64)      # where row b's next token goes
        if N == 0:
            return out, wpos
        cache = self.new_cache(B, S0 + N)
        logits = torch.empty(B, cfg.vocab_padded, device=dev, dtype=self.dtype)
        logits.copy_(self.prefill(tokens, cache, lens))
        u = torch.rand(N, B, generator=torch.Generator(device=dev).manual_seed(int(seed)), device=dev)
        # static buffers of the step
        u_buf = torch.empty(B, device=dev, dtype=torch.float32)
        cur = torch.empty(B, device=dev, dtype=torch.int64)
        done = torch.zeros(B, device=dev, dtype=torch.uint8)
        active = torch.ones(B, device=dev, dtype=torch.uint8)

        def pick():
            torch.bitwise_xor(done, 1, out=active)            # rows still running when the step begins
            ops.sample(logits, V, u_buf, float(temperature), k, p, done, stop, pad, out=cur)
            out.scatter_(1, wpos.unsqueeze(1), cur.unsqueeze(1))      # a finished row writes pad over pad
            wpos.add_(active)

        def step():
            pick()
            self.decode(cur, cache, active=active, out=logits)

        gc = None
        if use_graphs:
            from ..parallel.graphs import GraphCache
            gc = GraphCache("G")
        finished = False
        for i in range(N - 1):
            u_buf.copy_(u[i])
            if gc is None or i == 0:
                step()                       # with graphs: the warm-up, and one step of progress
            else:
                replay = "step" in gc
                gc.run("step", (), lambda _: step())
                if replay:
                    cache.pos += 1           # the captured decode counted its own step only
            if stop >= 0 and i % 16 == 15 and bool(done.all()):
                finished = True
                break
        if not finished:
            u_buf.copy_(u[N - 1])
            pick()
        return out, wpos

    @torch.no_grad()
    def generate_speculative(self, prompts, max_new_tokens: int, draft: "Generator", lookahead: int = 4,
                             pad_token: int = 0):
        """Greedy speculative decoding: ``(out, lengths, stats)`` with ``out`` / ``lengths`` as
        in :meth:`generate_batch` and ``stats = {"rounds", "drafted", "accepted"}``.

        ``draft`` is another :class:`Generator` over the same vocabulary.  Each round the
        draft decodes up to ``lookahead`` tokens greedily over its own ragged cache, the target
        runs one :meth:`extend` of those tokens behind its last one (``all_logits=True``),
        and per row the longest prefix of drafted tokens equal to the target's argmax is
        accepted, followed by the target's own next token; both caches are rolled back to the
        accepted length (:meth:`KVCache.truncate`).  The tokens are the target's own greedy
        continuation whatever the draft proposes; the draft only decides how many of them a
        round yields (1 to ``lookahead + 1``).

        Acceptance, the scatter into ``out`` and the new lengths are computed on the device.
        The tokens each row gained are read back to the host once per round -- one
        synchronisation per up to ``lookahead + 1`` tokens -- to bound ``cache.pos``, to give a
        row that has its ``max_new_tokens`` a count of 0 and to end the loop.  The last rounds
        draft fewer tokens, so that no row is asked for more than it may still emit.  Greedy
        only: there is no sampling variant."""
        cfg = self.cfg
        V, N, K, dev = cfg.vocab_size, int(max_new_tokens), int(lookahead), self.device
        if not isinstance(draft, Generator) or draft.cfg.vocab_size != V:
            raise ValueError("generate_speculative: the draft must be a Generator over the same vocabulary")
        if draft.device != dev:
            raise ValueError("generate_speculative: the draft lives on another device")
        rows = [torch.as_tensor(p).reshape(-1).to("cpu", torch.int64) for p in prompts]
        if not rows or any(r.numel() < 1 for r in rows):
            raise ValueError("generate_speculative: needs at least one prompt, each of at least one token")
        if N < 0 or K < 1:
            raise ValueError("generate_speculative: needs max_new_tokens >= 0 and lookahead >= 1")
        lens = [int(r.numel()) for r in rows]
        B, S0 = len(rows), max(lens)
        limit = min(cfg.max_seq_len, draft.cfg.max_seq_len)
        if S0 + N > limit:
            raise ValueError(f"generate_speculative: {S0} prompt + {N} new tokens exceed max_seq_len = {limit} "
                             "(the learned positions / RoPE table end there)")
        if any(int(r.min()) < 0 or int(r.max()) >= V for r in rows):
            raise ValueError(f"generate_speculative: prompt token outside the vocabulary [0, {V})")
        pad = int(pad_token)
        if not 0 <= pad < V:
            raise ValueError(f"generate_speculative: pad_token {pad} outside the vocabulary [0, {V})")

        tokens = torch.full((B, S0), pad, dtype=torch.int64)
        for b, r in enumerate(rows):
            tokens[b, : lens[b]] = r
        tokens = tokens.to(dev)
        W = S0 + N
        # K + 1 spare columns: a round writes its K + 1 candidates unmasked behind the row's
        # end; what lies beyond the final lengths is padded over at the end
        buf = torch.full((B, W + K + 1), pad, device=dev, dtype=torch.int64)
        buf[:, :S0] = tokens
        wpos = torch.tensor(lens, device=dev, dtype=torch.int64)
        stats = {"rounds": 0, "drafted": 0, "accepted": 0}
        if N == 0:
            return buf[:, :W].contiguous(), wpos, stats
        cap = min(W + K + 1, limit)
        tcache, dcache = self.new_cache(B, cap), draft.new_cache(B, cap)

        def greedy(lg):
            return lg[..., :V].float().argmax(-1)

        cur = greedy(self.prefill(tokens, tcache, lens))       # the target's first token: in no cache yet
        draft.prefill(tokens, dcache, lens)
        buf.scatter_(1, wpos[:, None], cur[:, None])
        wpos.add_(1)
        made = [1] * B                                  # tokens emitted per row (host)
        carry = [False] * B                             # the draft's cache lacks its own last token
        carry_tok = torch.full((B,), pad, device=dev, dtype=torch.int64)
        padcol = torch.full((B,), pad, device=dev, dtype=torch.int64)
        while True:
            rem = [N - m for m in made]
            live = [r > 0 for r in rem]
            if not any(live):
                break
            # host bounds of the lengths of the rows still running: every token but `cur`
            bound = max(lens[b] + made[b] - 1 for b in range(B) if live[b])
            tcache.pos = dcache.pos = bound
            k = min(K, max(rem) - 1, tcache.max_len - bound - 1, dcache.max_len - bound - 1)
            counts = [min(k + 1, r) for r in rem]
            drafts = []
            if k >= 1:
                # the draft catches up with `cur` (and with its own last token where every
                # draft of the last round was accepted), then decodes the rest one by one
                two = any(c and l for c, l in zip(carry, live))
                cflag = torch.tensor(carry, device=dev)
                if two:
                    tok = torch.stack([torch.where(cflag, carry_tok, cur), torch.where(cflag, cur, padcol)], 1)
                    c2 = [(2 if carry[b] else 1) if live[b] else 0 for b in range(B)]
                else:
                    tok, c2 = cur[:, None], [1 if l else 0 for l in live]
                d = greedy(draft.extend(tok, dcache, counts=c2))
                drafts.append(d)
                active = torch.tensor(live, device=dev).to(torch.uint8)
                for _ in range(k - 1):
                    d = greedy(draft.decode(d, dcache, active=active))
                    drafts.append(d)
            D = torch.stack(drafts, 1) if drafts else torch.empty(B, 0, device=dev, dtype=torch.int64)
            cnt = torch.tensor(counts, device=dev, dtype=torch.int64)
            base = tcache.lens.clone()
            a = greedy(self.extend(torch.cat([cur[:, None], D], 1), tcache, counts=counts, all_logits=True))
            # accepted drafts per row: the longest matching prefix, within the row's count
            m = (D == a[:, :k]).long().cumprod(1).sum(1)
            m = torch.minimum(m, (cnt - 1).clamp_(min=0))
            gain = torch.where(cnt > 0, m + 1, torch.zeros_like(m))
            buf.scatter_(1, wpos[:, None] + torch.arange(k + 1, device=dev)[None, :], a)
            wpos.add_(gain)
            cur = torch.where(cnt > 0, a.gather(1, m[:, None])[:, 0], cur)
            new_lens = base + gain.to(torch.int32)
            tcache.truncate(new_lens)
            if k >= 1:
                dcache.truncate(torch.minimum(dcache.lens, new_lens))
                carry_tok = D[:, k - 1]
            gained = gain.tolist()                      # the round's one host synchronisation
            for b in range(B):
                if live[b]:
                    made[b] += gained[b]
                    carry[b] = k >= 1 and gained[b] == k + 1
                    stats["drafted"] += counts[b] - 1
                    stats["accepted"] += gained[b] - 1
            stats["rounds"] += 1
        out = torch.where(torch.arange(W, device=dev)[None, :] < wpos[:, None], buf[:, :W], padcol[:, None])
        return out, wpos, stats
