"""Packed-document attention through the native models and the trainer on the GPU (bf16, the
kernels of attention_doc.hip): loss and gradients against the f32 autograd reference with the
same mask, the isolation of documents (exact), and HIP-graph / native-tape replay with
boundaries that change every step against eager steps."""
import pytest
import torch

import mipipe  # noqa: F401
from mipipe import ops
from mipipe.models import torch_ref
from mipipe.models.config import NativeConfig
from mipipe.models.native import MBContext, NativeModel

import attn_doc_refs as DR

pytestmark = pytest.mark.gpu

CFGS = {
    "gpt2": NativeConfig.gpt2("tiny", vocab_size=1000, d_model=256, n_layers=2, n_heads=4, d_ff=1024,
                              max_seq_len=256),
    "llama": NativeConfig.llama3("tiny", vocab_size=1000, d_model=256, n_layers=2, n_heads=4, n_kv_heads=2,
                                 d_ff=512, max_seq_len=256),
}
B, S = 2, 256
STARTS = [[0, 65, 128, 200], [0]]


def setup_module(module):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert ops.ext_available(), "HIP extension must be built for GPU tests"


def _docs(starts=STARTS, seq=S):
    return tuple(t.cuda() for t in DR.bounds_from_starts(seq, starts))


@pytest.mark.parametrize("name", list(CFGS))
def test_native_gpu_with_docs_vs_f32_reference(name):
    cfg = CFGS[name]
    model = NativeModel(cfg, 0, 1, "cuda", seed=1)
    g = torch.Generator().manual_seed(0)
    x = torch.randint(0, cfg.vocab_size, (B, S), generator=g)
    y = torch.randint(0, cfg.vocab_size, (B, S), generator=g)
    docs = _docs()
    P = {n: model.arena.w(n).float().cpu().clone().requires_grad_() for n in model.arena.order}
    ref = torch_ref.forward_loss(cfg, P, x, y, docs=tuple(t.cpu() for t in docs))
    ref.backward()
    ctx = MBContext(0, 1)
    loss = model.forward(x.cuda(), ctx, B, S, target=y.cuda(), docs=docs)
    model.backward(None, ctx, B, S)
    torch.cuda.synchronize()
    assert abs(loss.item() - ref.item()) < 2e-2 * abs(ref.item())
    for n in model.arena.order:
        gr = P[n].grad
        gg = model.arena.g(n).cpu()
        if n.startswith(("tok_embeddings", "output")):
            gr, gg = gr[: cfg.vocab_size], gg[: cfg.vocab_size]
        if gr.norm() < 1e-8:
            continue
        cos = torch.nn.functional.cosine_similarity(gr.flatten(), gg.flatten(), dim=0).item()
        rel = ((gr - gg).norm() / gr.norm()).item()
        assert cos > 0.99 and rel < 0.15, f"{name}:{n} cos={cos:.4f} rel={rel:.4f}"


@pytest.mark.parametrize("name", list(CFGS))
def test_documents_are_isolated_gpu(name):
    """Other tokens in document 0 (positions 0..64 of row 0) leave every later logits row
    bit-identical with ``docs``; without them the rows change."""
    cfg = CFGS[name]
    model = NativeModel(cfg, 0, 1, "cuda", seed=1)
    g = torch.Generator().manual_seed(2)
    x = torch.randint(0, cfg.vocab_size, (B, S), generator=g)
    x2 = x.clone()
    x2[0, :65] = torch.randint(0, cfg.vocab_size, (65,), generator=g)
    docs = _docs()

    def logits(tok, d):
        out = model.forward(tok.cuda(), MBContext(0, 1), B, S, docs=d)
        return out[:, : cfg.vocab_size].clone()

    a, b = logits(x, docs), logits(x2, docs)
    assert torch.equal(a[65:], b[65:])
    assert not torch.equal(a[:65], b[:65])
    a, b = logits(x, None), logits(x2, None)
    assert not torch.equal(a[65:S], b[65:S])
    assert torch.equal(a[S:], b[S:])     # row 1 never sees row 0


def _layouts(step):
    """Document starts of the 4 sequences of a batch: different at every step."""
    base = [[0, 65, 128, 200], [0], [0, 1, 2, 3, 100], [0, 192]]
    if step == 0:
        return base
    if step == 1:
        return [[0], list(range(0, 256, 16)), [0, 128], [0, 7, 250]]
    return [list(range(256)), [0, 64, 128, 192], [0], [0, 31]]


@pytest.mark.parametrize("recompute", [False, True])
def test_graph_replay_reads_refreshed_boundaries(recompute):
    from mipipe.engine import PipelineTrainer
    cfg = NativeConfig.gpt2("tiny", vocab_size=1000, d_model=256, n_layers=3, n_heads=4, d_ff=1024, max_seq_len=256)
    g = torch.Generator().manual_seed(0)
    x = torch.randint(0, 1000, (4, 256), generator=g).cuda()
    y = torch.randint(0, 1000, (4, 256), generator=g).cuda()
    steps = [_docs(_layouts(s)) for s in range(3)]
    res = {}
    for mode in ("eager", "graphs", "stale"):
        graphs = mode != "eager"
        tr = PipelineTrainer(cfg, pp=1, n_microbatches=2, mbs=2, seq_len=256, device=torch.device("cuda"),
                             recompute=recompute, graphs=graphs, seed=5, doc_mask=True)
        if graphs:
            tr.capture_graphs(x, y, docs=steps[0])
            assert tr.stages[0].graphs.captures >= 4
        # 'stale': the same graphs fed the first step's boundaries every time, to show that
        # the boundaries move the loss by more than the tolerance of the comparison
        res[mode] = [float(tr.train_step(x, y, docs=steps[0] if mode == "stale" else steps[s])) for s in range(3)]
        if mode == "graphs":
            nr = tr.runtime.native_runner
            assert tr.stages[0].graphs.replays >= 4
            assert nr is not None and nr.runs >= 2, tr.runtime.native_reason
    print("MEASURE losses", res)
    assert res["graphs"] == pytest.approx(res["eager"], rel=1e-4)
    moved = max(abs(a - b) / abs(a) for a, b in zip(res["graphs"][1:], res["stale"][1:]))
    assert moved > 1e-3, f"the boundaries change the loss by {moved:.2e} only: the comparison shows nothing"
