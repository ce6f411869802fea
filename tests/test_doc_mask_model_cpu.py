"""Packed-document attention through the model, the trainer and train.py (CPU, f32):
NativeModel with ``docs`` against the autograd reference, recompute on and off; the tokens
of one document cannot reach the logits of another; PP = 2 over gloo equals one process;
the construction and call errors; train.py with ``train.doc_eos``."""
import os
import subprocess
import sys

import pytest
import torch

import mipipe  # noqa: F401
from mipipe import ops
from mipipe.engine import PipelineTrainer
from mipipe.models import torch_ref
from mipipe.models.config import NativeConfig
from mipipe.models.native import MBContext, NativeModel

from dist_utils import run_world

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EOS = 3
CFGS = {
    "gpt2": lambda: NativeConfig.gpt2("tiny", vocab_size=100, d_model=64, n_layers=2, n_heads=4, d_ff=256, max_seq_len=32),
    "llama": lambda: NativeConfig.llama3("tiny", vocab_size=100, d_model=64, n_layers=2, n_heads=4, n_kv_heads=2,
                                         d_ff=128, max_seq_len=32),
}
B, S = 2, 16


def _data(vocab, rows=B, seq=S, seed=3):
    """Tokens without EOS except where placed: row 0 holds documents 0..4, 5..5, 6..10, 11..15;
    row 1 has an EOS at its last position only; every further row one at seq // 2."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(EOS + 1, vocab, (rows, seq), generator=g)
    y = torch.randint(0, vocab, (rows, seq), generator=g)
    x[0, 4], x[0, 5], x[0, 10] = EOS, EOS, EOS
    x[1, seq - 1] = EOS
    x[2:, seq // 2] = EOS
    return x, y


def _native(cfg, x, y, docs, recompute):
    model = NativeModel(cfg, 0, 1, "cpu", seed=5, dtype=torch.float32, recompute=recompute)
    ctx = MBContext(0, 11)
    loss = model.forward(x, ctx, x.shape[0], x.shape[1], target=y, docs=docs)
    model.backward(None, ctx, x.shape[0], x.shape[1])
    return model, float(loss)


@pytest.mark.parametrize("recompute", [False, True])
@pytest.mark.parametrize("name", list(CFGS))
def test_native_with_docs_matches_autograd(name, recompute):
    cfg = CFGS[name]()
    x, y = _data(cfg.vocab_size)
    docs = ops.doc_bounds(x, EOS)
    assert docs[0].reshape(B, S)[0].tolist() == [0] * 5 + [5] + [6] * 5 + [11] * 5
    model, loss = _native(cfg, x, y, docs, recompute)
    assert (model.recompute_layers > 0) == recompute
    P = {n: model.arena.master_view(n).clone().requires_grad_() for n in model.arena.order}
    ref = torch_ref.forward_loss(cfg, P, x, y, docs=docs)
    ref.backward()
    assert loss == pytest.approx(ref.item(), rel=1e-5)
    for n, p in P.items():
        got, g = model.arena.g(n), p.grad
        if n.startswith("tok_embeddings") or n.startswith("output"):
            got, g = got[: cfg.vocab_size], g[: cfg.vocab_size]
        torch.testing.assert_close(got, g, atol=2e-5, rtol=1e-4, msg=lambda m: f"{name}:{n}: {m}")
    # and the mask matters: the plain causal loss is another number
    plain = torch_ref.forward_loss(cfg, P, x, y)
    assert abs(plain.item() - ref.item()) > 1e-4


@pytest.mark.parametrize("name", list(CFGS))
def test_documents_are_isolated(name):
    """Two documents in a row: other tokens in the first leave the logits of the second
    exactly equal with ``docs``, and change them without."""
    cfg = CFGS[name]()
    g = torch.Generator().manual_seed(1)
    x = torch.randint(EOS + 1, cfg.vocab_size, (1, S), generator=g)
    x[0, 7] = EOS                        # documents 0..7 and 8..15
    x2 = x.clone()
    x2[0, :7] = torch.randint(EOS + 1, cfg.vocab_size, (7,), generator=g)
    assert not torch.equal(x, x2)
    model = NativeModel(cfg, 0, 1, "cpu", seed=5, dtype=torch.float32)

    def logits(tok, docs):
        out = model.forward(tok, MBContext(0, 11), 1, S, docs=docs)
        return out[:, : cfg.vocab_size].clone()

    docs = ops.doc_bounds(x, EOS)
    assert torch.equal(docs[0], ops.doc_bounds(x2, EOS)[0])
    a, b = logits(x, docs), logits(x2, docs)
    assert torch.equal(a[8:], b[8:])
    assert not torch.equal(a[:8], b[:8])
    a, b = logits(x, None), logits(x2, None)
    assert not torch.allclose(a[8:], b[8:], atol=1e-4)


# ------------------------------------------------------------------ trainer
M, MBS = 2, 2


def _train(name, pp, steps=2, recompute=False):
    cfg = CFGS[name]()
    tr = PipelineTrainer(cfg, pp=pp, schedule="1F1B", n_microbatches=M, mbs=MBS, seq_len=S, device=torch.device("cpu"),
                         dtype=torch.float32, lr=1e-3, layer_ranges=[(0, 1), (1, 2)] if pp == 2 else None,
                         head_align=8, doc_mask=True, recompute=recompute)
    losses = []
    for step in range(steps):
        x, y = _data(cfg.vocab_size, rows=M * MBS, seed=20 + step)
        x[2, 3 + step] = EOS             # boundaries move from step to step
        l = tr.train_step(x, y, docs=ops.doc_bounds(x, EOS))
        if l is not None:
            losses.append(float(l))
    return dict(losses=losses, sd={k: v.numpy().copy() for k, v in tr.state_dict().items()})


def _worker(rank, world, name):
    return _train(name, world)


@pytest.mark.parametrize("name", list(CFGS))
def test_pp2_doc_mask_matches_single_process(name):
    ref = _train(name, 1)
    res = run_world(_worker, 2, name)
    for r in res.values():
        if r["losses"]:
            assert r["losses"] == pytest.approx(ref["losses"], rel=1e-5)
        for k, w in r["sd"].items():
            torch.testing.assert_close(torch.from_numpy(w), torch.from_numpy(ref["sd"][k]), atol=1e-4, rtol=1e-4,
                                       msg=lambda m: f"{k}: {m}")


def test_trainer_doc_mask_changes_the_loss_and_matches_reference():
    """The trainer's first-step loss equals the reference's with the same mask (mean over the
    microbatches), and differs from the plain causal one."""
    cfg = CFGS["gpt2"]()
    x, y = _data(cfg.vocab_size, rows=M * MBS, seed=20)
    x[2, 3] = EOS
    docs = ops.doc_bounds(x, EOS)
    got = _train("gpt2", 1, steps=1)["losses"][0]
    tr = PipelineTrainer(cfg, pp=1, n_microbatches=M, mbs=MBS, seq_len=S, device=torch.device("cpu"),
                         dtype=torch.float32, lr=1e-3, head_align=8)
    P = {k: v.clone() for k, v in tr.state_dict().items()}
    ref = float(torch_ref.forward_loss(cfg, P, x, y, docs=docs))
    plain = float(torch_ref.forward_loss(cfg, P, x, y))
    assert got == pytest.approx(ref, rel=1e-5) and abs(ref - plain) > 1e-4


def test_construction_and_call_errors():
    cpu = torch.device("cpu")
    kw = dict(pp=1, n_microbatches=M, mbs=MBS, seq_len=S, dtype=torch.float32)
    ref = NativeConfig.reference(n_layers=2, n_heads=4, dim=64, vocab_size=100, dropout=0.0, dim_feedforward=128)
    with pytest.raises(ValueError, match="causal pre-norm"):
        PipelineTrainer(ref, device=cpu, doc_mask=True, **kw)
    drop = NativeConfig.gpt2("tiny", vocab_size=100, d_model=64, n_layers=2, n_heads=4, d_ff=256, max_seq_len=32,
                             dropout=0.1)
    with pytest.raises(ValueError, match="dropout"):
        PipelineTrainer(drop, device=cpu, doc_mask=True, **kw)
    # f32 on the GPU: refused before the device is touched
    with pytest.raises(ValueError, match="bf16"):
        PipelineTrainer(CFGS["gpt2"](), device=torch.device("cuda"), doc_mask=True, **kw)
    cfg = CFGS["gpt2"]()
    x, y = _data(cfg.vocab_size, rows=M * MBS)
    docs = ops.doc_bounds(x, EOS)
    on = PipelineTrainer(cfg, device=cpu, doc_mask=True, **kw)
    with pytest.raises(ValueError, match="docs"):
        on.train_step(x, y)
    with pytest.raises(ValueError, match="int32"):
        on.train_step(x, y, docs=(docs[0].long(), docs[1]))
    with pytest.raises(ValueError, match="entries"):
        on.train_step(x, y, docs=(docs[0][:-1], docs[1]))
    with pytest.raises(ValueError, match="docs"):
        on.capture_graphs(x, y)
    off = PipelineTrainer(cfg, device=cpu, **kw)
    with pytest.raises(ValueError, match="doc_mask=False"):
        off.train_step(x, y, docs=docs)
    # the model refuses docs on a block that is not a causal pre-norm decoder
    m = NativeModel(ref, 0, 1, "cpu", seed=5, dtype=torch.float32)
    with pytest.raises(ValueError):
        m.forward(x[:B], MBContext(0, 1), B, S, docs=(docs[0][: B * S], docs[1][: B * S]))
    with pytest.raises(ValueError):
        torch_ref.forward_loss(ref, {}, x[:B], y[:B], docs=docs)


def test_train_cli_with_doc_eos(tmp_path):
    mf = str(tmp_path / "m.jsonl")
    args = ["model.name=gpt2-tiny", "model.overrides.n_layers=2", "model.overrides.d_model=64",
            "model.overrides.n_heads=4", "model.overrides.d_ff=128", "model.overrides.vocab_size=8",
            "train.micro_batch=2", "train.seq_len=32", "train.log_every=1", "train.steps=2", "train.data=synthetic",
            f"train.doc_eos={EOS}", f"train.metrics_file={mf}", "parallel.pp=1", "parallel.microbatches=2"]
    env = dict(os.environ, OMP_NUM_THREADS="1", MIPIPE_DIST_BACKEND="gloo", MIPIPE_GLOO_GPU="0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train.py")] + args, capture_output=True, text=True,
                       timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    import json
    recs = [json.loads(line) for line in open(mf)]
    assert [rec["step"] for rec in recs] == [1, 2] and all(rec["loss"] > 0 for rec in recs)
