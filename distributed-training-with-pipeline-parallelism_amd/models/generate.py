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
"""
from __future__ import annotations

import dataclasses
from typing import List, Optional

import torch

from .. import ops
from .config import NativeConfig
from .native import Block, NativeModel


def _check_generative(cfg: NativeConfig) -> None:
    if cfg.cross_attn or not cfg.causal or not cfg.pre_norm:
        raise ValueError(f"{cfg.name}: generation needs a causal pre-norm decoder "
                         "(the reference post-LN cross-attention model is not a generator)")


class KVCache:
    """Per-layer K / V rows ``[B, max_len, Hkv * Dh]`` (K after RoPE) plus the number of
    valid rows: ``lens`` (int32 [B], on the device, what the decode kernel reads) and
    ``pos`` (the same number on the host; the sequences of a batch advance together)."""

    def __init__(self, cfg: NativeConfig, B: int, max_len: int, device, dtype=torch.bfloat16):
        if max_len < 1 or max_len > cfg.max_seq_len:
            raise ValueError(f"KVCache: max_len {max_len} outside [1, max_seq_len = {cfg.max_seq_len}]")
        self.B, self.max_len = int(B), int(max_len)
        self.device = torch.device(device)
        kv = cfg.n_kv_heads * cfg.head_dim
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

    def reset(self) -> None:
        self.lens.zero_()
        self.pos = 0
        self.ragged = False


class Generator:
    """KV-cache inference over one whole-model :class:`NativeModel` (``recompute=False``,
    dropout off: the training forward hands ``cfg.dropout`` to its kernels)."""

    def __init__(self, cfg: NativeConfig, device, dtype=torch.bfloat16, seed: int = 0, init: bool = True):
        _check_generative(cfg)
        cfg = dataclasses.replace(cfg, dropout=0.0)
        self._bind(NativeModel(cfg, 0, 1, torch.device(device), seed=seed, recompute=False, dtype=dtype, init=init))

    def _bind(self, model: NativeModel) -> None:
        self.model = model
        self.cfg = dataclasses.replace(model.cfg, dropout=0.0)
        self.arena = model.arena
        self.device = model.device
        self.dtype = model.arena.dtype
        self.blocks: List[Block] = model.blocks

    # ------------------------------------------------------------------ constructors
    @classmethod
    def from_model(cls, model: NativeModel) -> "Generator":
        """Wrap an existing single-stage model (``trainer.stages[0].model`` at ``pp = 1``).
        The weights are the model's arena itself: nothing is copied, and a later optimizer
        step is seen by the generator."""
        _check_generative(model.cfg)
        if model.num_stages != 1 or model.split_head:
            raise ValueError("Generator.from_model needs a single-stage model that owns its LM head (pp = 1)")
        self = cls.__new__(cls)
        self._bind(model)
        return self

    @classmethod
    def load(cls, path: str, device=None, dtype=None) -> "Generator":
        """Weights-only load of a checkpoint directory written by ``save_checkpoint`` at any
        PP / DP degree or head mode (the tensors are found by FQN).  Defaults: the GPU in
        bf16 when there is one, else the CPU in f32."""
        from ..utils.checkpoint import load_weights, read_manifest
        man = read_manifest(path)
        cfg = NativeConfig(**man["model"])
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else "cpu"
        device = torch.device(device)
        if dtype is None:
            dtype = torch.bfloat16 if device.type == "cuda" else torch.float32
        self = cls(cfg, device, dtype=dtype, init=False)
        load_weights([self.arena], path, strict=True)
        return self

    # ------------------------------------------------------------------ cache
    def new_cache(self, B: int, max_len: Optional[int] = None) -> KVCache:
        return KVCache(self.cfg, B, self.cfg.max_seq_len if max_len is None else max_len, self.device, self.dtype)

    # ------------------------------------------------------------------ layers
    def _norm(self, x, w, b):
        return ops.norm_fwd(x, w, b, kind=self.cfg.norm, eps=self.cfg.norm_eps)[0]

    def _ffn(self, blk: Block, x2: torch.Tensor) -> torch.Tensor:
        cfg = self.cfg
        h2 = self._norm(x2, blk.w("ffn_norm.weight"), blk.wb("ffn_norm.bias"))
        if cfg.activation == "swiglu":
            gu, _ = ops.linear(h2, blk.w("ffn.w13.weight"))
            y, _ = ops.linear(ops.swiglu_fwd(gu), blk.w("ffn.w2.weight"), residual=x2)
        else:
            g, _ = ops.linear(h2, blk.w("ffn.w1.weight"), blk.wb("ffn.w1.bias"), act=cfg.activation)
            y, _ = ops.linear(g, blk.w("ffn.w2.weight"), blk.wb("ffn.w2.bias"), residual=x2)
        return y

    def _qkv(self, blk: Block, x: torch.Tensor, S: int, pos: int) -> torch.Tensor:
        cfg = self.cfg
        h1 = self._norm(x, blk.w("attn_norm.weight"), blk.wb("attn_norm.bias"))
        qkv, _ = ops.linear(h1, blk.w("attn.wqkv.weight"), blk.wb("attn.wqkv.bias"))
        if cfg.pos == "rope":
            ops.rope_(qkv, blk.rope[0], blk.rope[1], S, cfg.n_heads, cfg.n_kv_heads, cfg.head_dim, pos_offset=pos)
        return qkv

    def _head(self, h: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Final norm + LM head of [B, D] rows -> logits [B, vocab_padded]."""
        A = self.arena
        if self.cfg.final_norm:
            h = self._norm(h, A.w("norm.weight"), A.w("norm.bias") if A.has("norm.bias") else None)
        logits, _ = ops.linear(h, self.model.head_weight(), A.w("output.bias") if A.has("output.bias") else None,
                               out=out)
        return logits

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
        for li, blk in enumerate(self.blocks):
            qkv = self._qkv(blk, x, S, 0)
            q, k, v = qkv[:, : H * Dh], qkv[:, H * Dh:(H + KV) * Dh], qkv[:, (H + KV) * Dh:]
            cache.k[li][:, :S].copy_(k.view(B, S, KV * Dh))     # after RoPE: rope_ is in place
            cache.v[li][:, :S].copy_(v.view(B, S, KV * Dh))
            o = torch.empty(B * S, H * Dh, device=x.device, dtype=x.dtype)
            lse = torch.empty(B * H * S, device=x.device, dtype=torch.float32)
            ops.attn_fwd(q, k, v, o, lse, B, S, S, H, KV, Dh, True, p_drop=0.0)
            x2, _ = ops.linear(o, blk.w("attn.wo.weight"), blk.wb("attn.wo.bias"), residual=x)
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
            qkv, _ = ops.linear(h1, blk.w("attn.wqkv.weight"), blk.wb("attn.wqkv.bias"))
            ops.rope_kv_append(qkv, blk.rope[0] if rope else None, blk.rope[1] if rope else None, cache.k[li],
                               cache.v[li], cache.positions, active, H, KV, Dh, rope=rope)
            o = torch.empty(B, H * Dh, device=x.device, dtype=x.dtype)
            ops.attn_decode(qkv[:, : H * Dh], cache.k[li], cache.v[li], cache.lens, o, H, KV, Dh,
                            max_len=cache.max_len)
            x2, _ = ops.linear(o, blk.w("attn.wo.weight"), blk.wb("attn.wo.bias"), residual=x)
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
        cache.lens.add_(1)            # the current token is a key too
        x = self._embed(tokens.to(self.device), 1, pos)
        for li, blk in enumerate(self.blocks):
            qkv = self._qkv(blk, x, 1, pos)
            q, k, v = qkv[:, : H * Dh], qkv[:, H * Dh:(H + KV) * Dh], qkv[:, (H + KV) * Dh:]
            cache.k[li][:, pos].copy_(k)
            cache.v[li][:, pos].copy_(v)
            o = torch.empty(B, H * Dh, device=x.device, dtype=x.dtype)
            ops.attn_decode(q, cache.k[li], cache.v[li], cache.lens, o, H, KV, Dh, max_len=pos + 1)
            x2, _ = ops.linear(o, blk.w("attn.wo.weight"), blk.wb("attn.wo.bias"), residual=x)
            x = self._ffn(blk, x2)
        cache.pos = pos + 1
        return self._head(x, out=out)

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
