"""Shared-prefix decode attention on the GPU: ops.decode_attn_shared_qkv
against a float64 attention over the gathered K/V, at the smallest shapes
where each piece can go wrong; forward_decode with and without a plan; one
engine run.

Every op case poisons what the kernels must not use with NaN: the cache
blocks no row owns (block-table padding points at one), the slots of each
row's last block past seq_len, the k/v columns of qkv and the workspace.
Heads 0..3 of every row look for a needle (q = 2 k_j, which outweighs any
other key by ~e^20): the last shared token, the first private one, the
first token of the second chunk and the appended token."""

import pytest
import torch

from attn_boundary_cases import BF16_TOL, BS, bad_rows, decode_oracle
from resilient_llm_amd import ops
from resilient_llm_amd.engine import LLMEngine, PagedKVCache, SamplingParams
from resilient_llm_amd.engine.kv_cache import shared_prefix_groups
from resilient_llm_amd.models import LlamaForCausalLM, get_config

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
D = 128
N_KV = 2
NAN = float("nan")


def device_plan(host, n_kv, chunks):
    T = len(host["tile_blocks"])
    return tuple(torch.tensor(host[k], dtype=torch.int32, device=DEV)
                 for k in ("n_shared", "row_tile", "row_slot", "tile_rows",
                           "tile_blocks", "tile_bt_row")) + (
        torch.full((T, n_kv, chunks, 64, D), NAN, device=DEV),
        torch.full((T, n_kv, chunks, 64, 2), NAN, device=DEV))


def run_case(groups, group_size, chunks, seed=0):
    """``groups``: [(shared blocks, [seq_len per member])]; the members of
    all groups are dealt into the batch round-robin.  Returns (got, want)
    as [B, n_q, D]."""
    g = torch.Generator().manual_seed(seed)
    n_q = N_KV * group_size
    order = sorted((i, gi) for gi, (_, lens) in enumerate(groups)
                   for i in range(len(lens)))
    lens = [groups[gi][1][i] for i, gi in order]
    B = len(lens)
    need = sum(s for s, _ in groups) + sum(-(-l // BS) for l in lens)
    perm = torch.randperm(need + 3, generator=g).tolist()
    shared = [[perm.pop() for _ in range(s)] for s, _ in groups]
    chains = [shared[gi][:] + [perm.pop() for _ in
                               range(-(-lens[r] // BS) - groups[gi][0])]
              for r, (_, gi) in enumerate(order)]
    poison = perm[0]                           # three blocks nobody owns
    bt = torch.full((B, max(map(len, chains)) + 2), poison, dtype=torch.int32)
    for r, c in enumerate(chains):
        bt[r, :len(c)] = torch.tensor(c, dtype=torch.int32)
    kc = torch.randn(need + 3, N_KV, BS, D, generator=g).to(torch.bfloat16)
    vc = torch.randn(need + 3, N_KV, BS, D, generator=g).to(torch.bfloat16)
    seq_lens = torch.tensor(lens, dtype=torch.int32)

    host = shared_prefix_groups(chains, [l - 1 for l in lens], BS, BS,
                                64 // group_size)
    q = torch.randn(B, n_q, D, generator=g)
    for r in range(B):
        ns = host["n_shared"][r]
        kv_tiles = (ns + 63) // 64
        second_chunk = (kv_tiles + chunks - 1) // chunks * 64
        targets = [ns - 1, ns, second_chunk, lens[r] - 1]
        for h, t in enumerate(targets):
            if 0 <= t < lens[r]:
                q[r, h] = 2 * kc[chains[r][t // BS], h // group_size,
                                 t % BS].float()
    q = q.to(torch.bfloat16)
    want = decode_oracle(q, kc, vc, bt, seq_lens, D ** -0.5)

    kc_p, vc_p = kc.clone(), vc.clone()
    for c in (kc_p, vc_p):
        c[perm[:3]] = NAN
        for r, chain in enumerate(chains):
            if lens[r] % BS:
                c[chain[-1], :, lens[r] % BS:] = NAN
    qkv = torch.full((B, (n_q + 2 * N_KV) * D), NAN, dtype=torch.bfloat16)
    qkv[:, :n_q * D] = q.reshape(B, -1)
    got = ops.decode_attn_shared_qkv(
        qkv.to(DEV), kc_p.to(DEV), vc_p.to(DEV), bt.to(DEV),
        seq_lens.to(DEV), device_plan(host, N_KV, chunks), D ** -0.5, n_q)
    return got.cpu().view(B, n_q, D), want


def check(got, want):
    err = (got.double() - want).abs().max().item()
    print(f"max abs err {err:.3e}")
    bad = bad_rows(got, want, BF16_TOL, BF16_TOL)
    assert not bad.any(), (bad.nonzero().flatten().tolist(), err)


def test_one_shared_block():
    check(*run_case([(1, [17, 31])], 4, 1))


@pytest.mark.parametrize("blocks", [4, 5, 9])
@pytest.mark.parametrize("chunks", [1, 2, 3])
def test_kv_tiles_and_chunks(blocks, chunks):
    n = blocks * BS
    check(*run_case([(blocks, [n + 1, n + 16, n + 40])], 4, chunks))


@pytest.mark.parametrize("members,group_size", [(16, 4), (17, 4), (9, 8)])
def test_row_tiles(members, group_size):
    lens = [5 * BS + 1 + (7 * i) % 33 for i in range(members)]
    check(*run_case([(5, lens)], group_size, 2))


def test_two_groups_and_a_loner_interleaved():
    # the short group's chunks 1 and 2 lie past its prefix (l = 0)
    check(*run_case([(9, [145, 160, 170, 200]), (2, [33, 50, 64]),
                     (0, [70])], 4, 3))


def test_heuristic_and_wrapper_checks():
    assert ops.shared_prefix_chunks(1, 8, 128) == 32
    assert ops.shared_prefix_chunks(1, 8, 16) == 16      # one per KV tile
    assert ops.shared_prefix_chunks(64, 8, 128) == 1
    host = shared_prefix_groups([[0, 1], [0, 2]], [17, 17], BS, BS, 16)
    plan = device_plan(host, 1, 1)
    kc = torch.zeros(4, 1, BS, D, dtype=torch.bfloat16, device=DEV)
    qkv = torch.zeros(2, 6 * D, dtype=torch.bfloat16, device=DEV)
    bt = torch.tensor([[0, 1], [0, 2]], dtype=torch.int32, device=DEV)
    sl = torch.tensor([18, 18], dtype=torch.int32, device=DEV)
    ops.decode_attn_shared_qkv(qkv, kc, kc, bt, sl, plan, 1.0, 4)
    fp8 = kc.to(torch.float8_e4m3fn)
    bs8 = kc[:, :, :8].contiguous()
    d64 = kc[..., :64].contiguous()
    for bad in (
            lambda: ops.decode_attn_shared_qkv(qkv, fp8, fp8, bt, sl, plan,
                                               1.0, 4),
            lambda: ops.decode_attn_shared_qkv(qkv, bs8, bs8, bt, sl, plan,
                                               1.0, 4),
            lambda: ops.decode_attn_shared_qkv(
                qkv[:, :6 * 64].contiguous(), d64, d64, bt, sl, plan, 1.0, 4),
            lambda: ops.decode_attn_shared_qkv(
                qkv[:, :3 * D].contiguous(), kc, kc, bt, sl, plan, 1.0, 1),
            lambda: ops.decode_attn_shared_qkv(qkv[:1], kc, kc, bt[:1],
                                               sl[:1], plan, 1.0, 4)):
        with pytest.raises(RuntimeError):
            bad()


# ------------------------------------------------------- model and engine
def make_engine(device, dtype, num_blocks=64, **kw):
    cfg = get_config("tiny-128")
    model = LlamaForCausalLM(cfg, device=device, dtype=dtype, seed=3)
    kv = PagedKVCache.for_model(cfg, num_blocks, device=device,
                                kv_dtype=dtype)
    return LLMEngine(model, kv, enable_prefix_caching=False, **kw)


def test_forward_decode_with_plan_stays_within_twice_the_bf16_gap():
    """The state: four forks of an 80-token prompt, prefilled by the
    engine.  Reference: forward_decode in float32 on the CPU over the same
    weights and cache.  The plan path may be at most twice as far from it
    as the existing path is."""
    e = make_engine(DEV, torch.bfloat16, shared_prefix_attention=True,
                    shared_prefix_min_tokens=16)
    rids = [f"g.c{i}" for i in range(4)]
    e.add_request_group(rids, [5 + (7 * i) % 90 for i in range(80)],
                        [SamplingParams(max_tokens=8, temperature=0.9,
                                        seed=10 + i) for i in range(4)])
    while not e.stats["shared_prefix_steps"]:
        e.step()
    plan, n_rows = e._b_shared_plan
    assert n_rows == 4
    pos = e._b_pos.clone()
    blk = (pos // BS).long()
    slots = e._b_bt.gather(1, blk.unsqueeze(1)).squeeze(1) * BS + pos % BS
    k0, v0 = e.kv.k.clone(), e.kv.v.clone()

    def logits(model, kv, dev, **kw):
        args = [t.to(dev) for t in (e._b_ids, pos, slots, e._b_bt, pos + 1)]
        return model.forward_decode(args[0], args[1], kv, *args[2:],
                                    **kw).float().cpu()

    with_plan = logits(e.model, e.kv, DEV, shared_plan=plan)
    assert torch.isfinite(e.kv.k).all()
    e.kv.k.copy_(k0)
    e.kv.v.copy_(v0)
    plain = logits(e.model, e.kv, DEV)

    cpu = make_engine("cpu", torch.float32)
    for name, w in e.model.params.items():
        cpu.model.params[name] = w.float().cpu()
    cpu.kv.k, cpu.kv.v = k0.float().cpu(), v0.float().cpu()
    want = logits(cpu.model, cpu.kv, "cpu")
    gap_plain = (plain - want).abs().max().item()
    gap_plan = (with_plan - want).abs().max().item()
    print(f"logits gap to f32: existing {gap_plain:.4e}, "
          f"shared {gap_plan:.4e}")
    assert gap_plain > 0 and gap_plan <= 2 * gap_plain


def test_engine_group_completes_and_frees_every_block():
    e = make_engine(DEV, torch.bfloat16, shared_prefix_attention=True,
                    shared_prefix_min_tokens=16)
    rids = [f"g.c{i}" for i in range(4)]
    e.add_request_group(rids, [5 + (7 * i) % 90 for i in range(80)],
                        [SamplingParams(max_tokens=12, temperature=0.8,
                                        seed=100 + i) for i in range(4)])
    outs = {}
    for _ in range(200):
        if not e.has_work():
            break
        for o in e.step():
            outs.setdefault(o.req_id, []).append(o.token_id)
    assert not e.has_work() and sorted(outs) == rids
    assert e.kv.free_blocks == e.kv.num_blocks
    assert e.stats["shared_prefix_steps"] > 0
    assert e.stats["shared_prefix_rows"] >= 2 * e.stats["shared_prefix_steps"]
