"""FusedEmbeddingOptimizer (models/fused_embedding.py) without a GPU: the
torch-op fallback against an fp64 dense reference and against torch.optim,
the API contract, and the DDP example's argument check."""

import importlib.util
import os

import pytest
import torch

from ray_shuffling_data_loader_amd.models import fused_embedding as fe
from test_fused_embedding_cpu import (
    backward_ref64,
    exact_dout,
    make_indices,
    make_tables,
)

KINDS = ("sgd", "adagrad", "rowwise_adagrad")
LR, EPS = 0.05, 1e-3


def f32(v):
    return torch.tensor(v, dtype=torch.float32).double()


def make_opt(kind, tables, seed=7, **kw):
    """An optimizer over ``tables`` whose state is random with sum > 0."""
    kw = {"lr": LR, "eps": EPS, **kw}
    opt = fe.FusedEmbeddingOptimizer(tables, kind=kind, **kw)
    g = torch.Generator().manual_seed(seed)
    for st in opt.state.values():
        for h in st.values():
            h.copy_(torch.rand(h.shape, generator=g) + 0.1)
    return opt


def run_step(opt, idx, tables, dout):
    fe.fused_embedding(idx, tables, optimizer=opt).backward(dout)
    opt.step()


def reference_step64(kind, idx, tables, sums, dout, lr=LR, eps=EPS):
    """One dense step of the class docstring's formulas in fp64 over all
    rows: (p', u = p - p', touched row mask) per table."""
    g64, cnt, _ = backward_ref64(idx, tables, dout)
    out = []
    for w, h, g, n in zip(tables, sums, g64, cnt):
        p = w.detach().double().cpu()
        if kind == "sgd":
            u = f32(lr) * g
        else:
            h = h.double().cpu()
            h = h + g * g if kind == "adagrad" else (
                h + (g * g).mean(1))[:, None]
            u = f32(lr) * (g / (h.sqrt() + f32(eps)))
        out.append((p - u, u, n[:, 0] > 0))
    return out


def step_bound(D, u, p_new):
    """2^-24 * ((D + 8) |u| + 2 |p'|): the longest rounding chain is
    rowwise_adagrad's D squares and adds, the add into h, sqrt, + eps,
    divide, times lr, subtract."""
    return 2.0**-24 * ((D + 8) * u.abs() + 2 * p_new.abs())


@pytest.mark.parametrize("kind", KINDS)
def test_fallback_against_fp64_reference(kind):
    B, D, cards = 97, 16, (3, 17, 300)
    idx = make_indices(B, cards, "cpu")
    tables = make_tables(cards, D, "cpu")
    before = [w.detach().clone() for w in tables]
    opt = make_opt(kind, tables)
    sums = [st.get("sum") for st in opt.state.values()]
    sums0 = [None if h is None else h.clone() for h in sums]
    dout = exact_dout(B, len(cards) * D, "cpu")
    ref = reference_step64(kind, idx, tables, sums0, dout)
    run_step(opt, idx, tables, dout)
    assert opt.step_count == 1
    for w, w0, h, h0, (p, u, hit) in zip(tables, before, sums, sums0, ref):
        err = (w.detach().double() - p).abs()
        bound = step_bound(D, u, p)
        print(kind, "max err", err.max().item(), "bound", bound.max().item())
        assert (err <= bound).all()
        assert hit.any() and torch.equal(w.detach()[~hit], w0[~hit])
        if h is not None:
            assert torch.equal(h[~hit], h0[~hit])
            assert (h[hit] > h0[hit]).any()


@pytest.mark.parametrize("kind", ("sgd", "adagrad"))
def test_three_steps_match_torch_optim(kind):
    B, D, cards = 97, 16, (3, 17, 300)
    tables = make_tables(cards, D, "cpu")
    dense = [w.detach().clone().requires_grad_() for w in tables]
    before = [w.detach().clone() for w in tables]
    opt = fe.FusedEmbeddingOptimizer(
        tables, kind=kind, lr=LR, eps=EPS, initial_accumulator_value=0.5)
    if kind == "sgd":
        ref = torch.optim.SGD(dense, lr=LR)
    else:
        ref = torch.optim.Adagrad(dense, lr=LR, eps=EPS,
                                  initial_accumulator_value=0.5)
    tol = [torch.zeros_like(w, dtype=torch.float64) for w in tables]
    hit = [torch.zeros(c, dtype=torch.bool) for c in cards]
    for step in range(3):
        idx = make_indices(B, cards, "cpu", seed=10 + step)
        dout = exact_dout(B, len(cards) * D, "cpu", seed=20 + step)
        run_step(opt, idx, tables, dout)
        old = [w.detach().clone() for w in dense]
        ref.zero_grad(set_to_none=True)
        fe.fused_embedding(idx, dense).backward(dout)  # dense index_add_
        ref.step()
        for t, (w, w0) in enumerate(zip(dense, old)):
            tol[t] += step_bound(D, (w0 - w.detach()).double(),
                                 w.detach().double())
            hit[t] |= w.grad.abs().sum(1) > 0
    for t, (w, d) in enumerate(zip(tables, dense)):
        err = (w.detach().double() - d.detach().double()).abs()
        print(kind, t, "max err", err.max().item(), "tol", tol[t].max().item())
        assert (err <= tol[t]).all()
        assert torch.equal(w.detach()[~hit[t]], before[t][~hit[t]])
        if kind == "adagrad":
            assert (opt.state[t]["sum"][~hit[t]] == 0.5).all()
            torch.testing.assert_close(
                opt.state[t]["sum"], ref.state[d]["sum"], rtol=2.0**-22,
                atol=0)


def test_api_contract(monkeypatch):
    B, D, cards = 33, 8, (3, 40)
    idx = make_indices(B, cards, "cpu")
    tables = make_tables(cards, D, "cpu")
    dout = exact_dout(B, len(cards) * D, "cpu")
    opt = make_opt("adagrad", tables)
    with pytest.raises(ValueError, match="other tables"):
        fe.fused_embedding(idx, make_tables(cards, D, "cpu"), optimizer=opt)
    with pytest.raises(ValueError, match="eps"):
        fe.FusedEmbeddingOptimizer(tables, kind="adagrad", eps=0.0)
    with pytest.raises(ValueError, match="kind"):
        fe.FusedEmbeddingOptimizer(tables, kind="adam")
    with pytest.raises(RuntimeError, match="no pending batch"):
        opt.step()
    versions = [w._version for w in tables]
    fe.fused_embedding(idx, tables, optimizer=opt).backward(dout)
    assert all(w.grad is None for w in tables)
    with pytest.raises(RuntimeError, match="second backward"):
        fe.fused_embedding(idx, tables, optimizer=opt).backward(dout)
    opt.zero_grad()
    with pytest.raises(RuntimeError, match="no pending batch"):
        opt.step()
    fe.fused_embedding(idx, tables, optimizer=opt).backward(dout)
    monkeypatch.setattr(torch.distributed, "is_initialized", lambda: True)
    monkeypatch.setattr(torch.distributed, "get_world_size", lambda: 2)
    with pytest.raises(RuntimeError, match="more than one process"):
        opt.step()
    monkeypatch.undo()
    opt.step()
    assert all(w._version > v for w, v in zip(tables, versions))
    assert opt.state[0]["sum"].shape == (3, D)
    rw = fe.FusedEmbeddingOptimizer(tables, kind="rowwise_adagrad",
                                    initial_accumulator_value=0.25)
    assert rw.state[1]["sum"].shape == (40,)
    assert (rw.state[1]["sum"] == 0.25).all()
    assert fe.FusedEmbeddingOptimizer(tables).state[0] == {}


@pytest.mark.parametrize("kind", KINDS)
def test_state_dict_round_trip_resumes_exactly(kind):
    B, D, cards = 33, 16, (3, 40, 300)
    tables = make_tables(cards, D, "cpu")
    opt = make_opt(kind, tables)
    batches = [
        (make_indices(B, cards, "cpu", seed=30 + s),
         exact_dout(B, len(cards) * D, "cpu", seed=40 + s))
        for s in range(2)
    ]
    run_step(opt, batches[0][0], tables, batches[0][1])
    resumed = [w.detach().clone().requires_grad_() for w in tables]
    other = fe.FusedEmbeddingOptimizer(resumed, kind="sgd", lr=1.0)
    other.load_state_dict(opt.state_dict())
    assert (other.kind, other.lr, other.eps, other.step_count) == (
        kind, LR, EPS, 1)
    run_step(opt, batches[1][0], tables, batches[1][1])
    run_step(other, batches[1][0], resumed, batches[1][1])
    for t, (a, b) in enumerate(zip(tables, resumed)):
        assert torch.equal(a, b)
        for s in opt.state[t]:
            assert torch.equal(opt.state[t][s], other.state[t][s])


def test_train_ddp_embedding_optimizer_arguments():
    path = os.path.join(
        os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
        "examples", "ddp", "train_ddp.py",
    )
    spec = importlib.util.spec_from_file_location("_train_ddp_example", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    for argv in (["--embedding-optimizer", "adagrad"],
                 ["--embedding-optimizer", "sgd", "--spec", "tabular"]):
        with pytest.raises(SystemExit, match="--fused-embedding"):
            mod.parse_args(argv)
    args = mod.parse_args(["--embedding-optimizer", "rowwise-adagrad",
                           "--spec", "tabular", "--fused-embedding"])
    assert args.embedding_optimizer == "rowwise-adagrad"
    assert mod.parse_args([]).embedding_optimizer == "torch"
