"""CPU, world_size 2, gloo: the replica-parallel path (autosmoothquant_amd/replica.py) --
row sharding, the one-time broadcast of the quantised buffers, the post-broadcast fingerprint,
and 'every replica's rows == the single-process rows bit for bit' (the oracle stands in for the
HIP compute, which needs a GPU; the sharding/collective logic under test is device-agnostic)."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import detrng


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _make_model(seed):
    from autosmoothquant_amd.layers.nn.linear import (W8A8BFP32OFP32Linear, W8A8BFP32OFP32LinearWithQuantScale,
                                                      W8A8BFP32OFP32QKVLinear, FP8LinearStatic, FP8LinearDynamic, FP8E5M2Linear, FP8LinearMX)
    g = torch.Generator().manual_seed(seed)
    mods = torch.nn.ModuleDict()
    a = W8A8BFP32OFP32Linear(64, 48, True, "per-tensor")
    b = W8A8BFP32OFP32LinearWithQuantScale(48, 64, False, "per-tensor")
    c = W8A8BFP32OFP32QKVLinear([32, 16, 16], 64, 64, True, "per-token")
    for m in (a, b, c):
        m.weight = torch.randint(-128, 128, m.weight.shape, generator=g, dtype=torch.int8)
        if m.use_bias:
            m.bias = torch.randn(m.out_features, generator=g)
    a.dequant_scale = torch.tensor(0.001 * (seed + 1))
    b.dequant_scale = torch.tensor(0.002 * (seed + 1))
    b.quant_scale = torch.tensor(0.5 + seed)
    c.q_dequant_scale, c.k_dequant_scale, c.v_dequant_scale = (torch.tensor(0.003 * (seed + 1) * (i + 1)) for i in range(3))
    mods["a"], mods["b"], mods["c"] = a, b, c
    # fp8 classes travel in the same arena (weights as raw fp8 bytes, their host scalars in the tail)
    d = FP8LinearStatic(32, 24, use_bias=True)
    e = FP8LinearDynamic(24, 40, "per-token")
    f = FP8E5M2Linear(40, 8, use_bias=False)
    for m in (d, e, f):
        m.weight = torch.randint(0, 120, m.weight.shape, generator=g, dtype=torch.uint8).view(m._weight_dtype)
    d.bias = torch.randn(24, generator=g)
    d.weight_scale, d.input_scale, d.output_scale = torch.tensor(0.01 * (seed + 1)), torch.tensor(0.02 * (seed + 2)), torch.tensor(0.0)
    e.weight_scale = torch.tensor(0.04 * (seed + 3))
    mods["d"], mods["e"], mods["f"] = d, e, f
    h = FP8LinearMX(64, 16, use_bias=True)   # the MX opt-in: its block-scale bytes are a third device buffer of the arena
    h.weight = torch.randint(0, 120, h.weight.shape, generator=g, dtype=torch.uint8).view(h._weight_dtype)
    h.weight_scale_mx = torch.randint(100, 140, h.weight_scale_mx.shape, generator=g, dtype=torch.uint8)
    h.bias = torch.randn(16, generator=g)
    mods["h"] = h
    return mods


def _oracle_forward(mods, x):
    """x [M,64] f32 -> y [M,48] through module a, with the oracle as the compute"""
    from oracle import w8a8 as O
    a = mods["a"]
    return O.linear_forward(x, "f32", a.weight.numpy(), float(a.dequant_scale), a.bias.numpy(), a.act_quant)


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from autosmoothquant_amd import replica
        mods = _make_model(seed=0 if rank == 0 else 7)  # non-source ranks start from different buffers
        fp_before = replica.buffers_fingerprint(mods)
        differs_before = not replica.all_ranks_equal(fp_before)
        nbytes = replica.broadcast_quantized(mods, src=0)
        fp = replica.buffers_fingerprint(mods)
        same_after = replica.all_ranks_equal(fp)
        # scalar scales stay host-side fp32 after the broadcast
        host_ok = all(m._buffers[n].device.type == "cpu" and m._buffers[n].dtype == torch.float32
                      for m in mods.values() for n in m._host_scalars)
        # module buffers are views of ONE flat arena afterwards, dtypes / shapes untouched
        arena = mods._asq_arena
        base = arena.buf.untyped_storage().data_ptr()
        host_ok = host_ok and all(m.weight.untyped_storage().data_ptr() == base for m in mods.values())
        host_ok = host_ok and mods["d"].weight.dtype == torch.float8_e4m3fn and mods["f"].weight.dtype == torch.float8_e5m2
        host_ok = host_ok and mods["h"].weight_scale_mx.dtype == torch.uint8 and mods["h"].weight_scale_mx.untyped_storage().data_ptr() == base
        host_ok = host_ok and arena.total % (256 * world) == 0
        # each rank computes its shard of a global batch; rank 0 gathers and compares with the 1-process result
        M = 37
        xg = detrng.act_like(5, 0, (M, 64), scale=40.0)
        lo, hi = replica.shard_rows(M, world, rank)
        y_local = torch.from_numpy(_oracle_forward(mods, xg[lo:hi]))
        parts = [None] * world
        dist.all_gather_object(parts, (lo, hi, y_local.numpy()))
        q.put((rank, differs_before, same_after, host_ok, nbytes, fp, parts if rank == 0 else None))
    finally:
        dist.destroy_process_group()


def test_shard_rows_partition():
    from autosmoothquant_amd import replica
    for M in (0, 1, 7, 256, 1000):
        for G in (1, 2, 3, 8):
            spans = [replica.shard_rows(M, G, r) for r in range(G)]
            assert spans[0][0] == 0 and spans[-1][1] == M
            assert all(spans[i][1] == spans[i + 1][0] for i in range(G - 1))
            assert max(h - l for l, h in spans) - min(h - l for l, h in spans) <= 1
    with pytest.raises(ValueError):
        replica.shard_rows(4, 2, 2)


@pytest.mark.timeout(300)
def test_broadcast_and_row_sharding_world2():
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=240) for _ in range(world)), key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    fps = set()
    for rank, differs_before, same_after, host_ok, nbytes, fp, parts in res:
        assert differs_before, "test is vacuous if ranks start identical"
        assert same_after and host_ok
        # int8 weights + fp8 weights + fp32 biases + (6 int8-module + 4 fp8-module) host scalars + the MX module (weight, block scales, bias)
        assert nbytes == (48 * 64 + 64 * 48 + 64 * 64) + (24 * 32 + 40 * 24 + 8 * 40) + 4 * (48 + 64 + 24) + 4 * (6 + 4) + (16 * 64 + 16 * 2 + 4 * 16)
        fps.add(fp)
    assert len(fps) == 1
    # replica rows == single-process rows, bit for bit
    ref_mods = _make_model(seed=0)
    xg = detrng.act_like(5, 0, (37, 64), scale=40.0)
    ref = _oracle_forward(ref_mods, xg)
    got = np.concatenate([p[2] for p in sorted(res[0][6], key=lambda t: t[0])], axis=0)
    assert np.array_equal(got, ref)


def _worker_edge(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from autosmoothquant_amd import replica
        # A. one rank found no quantised module: every rank must RAISE the structure mismatch (round 2: that rank returned early and the
        #    others hung in the signature all-reduce)
        mods = _make_model(seed=rank) if rank != 2 else torch.nn.ModuleDict()
        try:
            replica.broadcast_quantized(mods, src=0)
            raised = False
        except RuntimeError as e:
            raised = "different module structures" in str(e)
        # B. a sub-group whose source is not its first member: `src` is a global rank, chunk indices are group ranks
        sub = dist.new_group([1, 2])
        same = None
        if rank in (1, 2):
            m2 = _make_model(seed=10 + rank)
            want = replica.buffers_fingerprint(_make_model(seed=12))
            replica.broadcast_quantized(m2, src=2, group=sub)
            same = replica.buffers_fingerprint(m2) == want and float(m2["a"].dequant_scale) == pytest.approx(0.001 * 13)
        q.put((rank, raised, same))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_broadcast_mismatch_raises_everywhere_and_subgroup_source_world3():
    world = 3
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker_edge, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=240) for _ in range(world)), key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert all(r[1] for r in res), "every rank must raise the structure mismatch (no hang, no silent return)"
    assert res[1][2] is True and res[2][2] is True and res[0][2] is None


def _mixtral(seed):
    from autosmoothquant_amd import harness
    torch.manual_seed(seed)
    fl = harness.MixtralLayer(64, 96, 4, 2, experts=4, top_k=2)
    with torch.no_grad():
        for p in fl.parameters():
            if p.dim() == 2:
                p.copy_(torch.randn(p.shape) * 0.05)
    scales = {"attn_in": 0.05, "o_in": 0.05, "mlp_in": 0.05, "down_in": [0.05 + 0.01 * seed, 0.06, 0.07, 0.08]}
    return harness.to_w8a8_mixtral(fl, scales)


def _worker_mixtral(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from autosmoothquant_amd import replica
        from autosmoothquant_amd.layers.nn.linear import W8A8BFP32OFP32Linear
        layer = _mixtral(seed=0 if rank == 0 else 5)
        lin = W8A8BFP32OFP32Linear(64, 48, False, "per-tensor")
        lin.weight = torch.randint(-128, 128, (48, 64), generator=torch.Generator().manual_seed(rank), dtype=torch.int8)
        root = torch.nn.ModuleDict({"layer": layer, "lin": lin})
        assert layer._stacks_current()
        # a cached offset image on every rank (a stand-in builder: a real one needs a HIP device; the KEY logic under test is device-agnostic)
        torch.cuda.is_current_stream_capturing = lambda: False   # (this worker has no device to ask)
        builds = []
        image = lambda w, out=None: builds.append(w.data_ptr()) or (torch.zeros_like(w), torch.zeros(w.shape[0], 2, dtype=torch.int32))
        assert lin.image.get((lin.weight,), image) is lin.image.get((lin.weight,), image) and len(builds) == 1
        key_before = lin.image.key
        st_ptr = layer._w1_stack.data_ptr()
        nbytes = replica.broadcast_quantized(root, src=0)
        fp = replica.buffers_fingerprint(root)
        fps = replica.gather_fingerprints(fp)
        # 1. the per-expert buffers were re-homed into the arena: the stacks are stale until moe() restacks, and their image key with them
        stale = not layer._stacks_current()
        layer.stack_experts()
        restacked = layer._stacks_current() and layer._w1_stack.data_ptr() != st_ptr
        # 2. the module's cached image is keyed on the weight's storage: the arena view is a different storage -> the next offset_image() rebuilds it
        lin.image.get((lin.weight,), image)
        key_moved = lin.image.key != key_before and len(builds) == 2
        q.put((rank, nbytes, fp, fps, stale, restacked, key_moved, [float(e.w2.dequant_scale) for e in layer.experts], layer._w2_scale.tolist()))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_broadcast_mixtral_layer_and_image_keys_world2():
    """a Mixtral layer (expert stacks) and a module with a cached offset image through the arena broadcast: every rank ends with rank 0's
    experts, the stacks are rebuilt from the re-homed buffers, the image cache key no longer matches (so the receiver rebuilds the image), and the per-rank
    fingerprints bench.py prints are equal."""
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker_mixtral, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=240) for _ in range(world)), key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    ref = _mixtral(0)
    want_scales = [float(e.w2.dequant_scale) for e in ref.experts]
    for rank, nbytes, fp, fps, stale, restacked, key_moved, scales, stack_scales in res:
        assert nbytes > 0 and stale and restacked and key_moved
        assert fps == [res[0][2]] * world and fp == res[0][2]
        assert scales == want_scales and stack_scales == pytest.approx(want_scales)
