"""GPU (-m gpu): harness.concurrent_linears runs same-input modules of equal width as ONE split-output launch over their stacked offset images
(ASQ_EPI_OUT_SPLIT; ASQ_MERGE_LINEARS, default on) and returns what the modules' own forwards return, bit for bit.

Two module shapes, K = 256 in both:
  M = 1280, N = 4608   the shape of tests/test_hip_out_split.py.  A single module of this size is below the 256 x 256 kernel class (90 tiles), so it holds no
                       offset image, its activation carries no row offsets and the run is NOT merged: the per-module path must be what runs, unchanged.
  M = 2304, N = 4096   the smallest llama-like module that holds an image (144 tiles): three of them merge into one persistent launch of 432 tiles.
The number of merged launches is counted, so a test cannot pass by silently taking the other path."""
import pytest
import torch

from autosmoothquant_amd import harness, ops
from autosmoothquant_amd.layers.nn.linear import W8A8BFP32OFP32Linear, W8A8BFP32OFP32LinearWithQuantScale

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
K = 256
SMALL, BIG = (1280, 4608), (2304, 4096)
N2 = 4352       # a second width that holds an image at 2304 rows (153 tiles)


def module(N, seed, cls=W8A8BFP32OFP32Linear, act_quant="per-tensor", bias=False):
    g = torch.Generator().manual_seed(seed)
    m = cls(K, N, bias, act_quant)
    m.weight = torch.randint(-128, 128, (N, K), generator=g, dtype=torch.int8)
    if bias:
        m.bias = torch.randn(N, generator=g)
    m.dequant_scale = torch.tensor(1e-4 * (1 + seed % 5))
    return m.to(DEV)


def activation(M, mods, seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = (torch.randn(2, M // 2, K, generator=g, device=DEV) * 30).half()
    return mods[0].quantize_input(x, consumers=mods)


def plain_reference(mods, xi):
    """the modules' outputs from the plain operands alone: no offset image, nothing the merged path shares"""
    xq = xi.plain_xq()
    return [ops.linear_w8a8(xq, m.weight, xi.out_dtype, m._scalar("dequant_scale"), xi.s_row, None, m.bias.clone() if m.use_bias else None).view(*xi.lead, m.out_features)
            for m in mods]


@pytest.fixture
def merged_calls(monkeypatch):
    """counts the split-output launches"""
    calls, real = [], ops.linear_w8a8_off

    def counted(*a, **kw):
        if kw.get("out_split"):
            calls.append(kw["out_split"])
        return real(*a, **kw)
    monkeypatch.setattr(ops, "linear_w8a8_off", counted)
    monkeypatch.setattr(harness, "merge_linears_enabled", True)
    return calls


def equal_lists(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and x.dtype == y.dtype and x.is_contiguous() and torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("shape,launches", [(SMALL, []), (BIG, [3])], ids=["1280x4608", "2304x4096"])
@pytest.mark.parametrize("act_quant", ["per-tensor", "per-token"])
def test_equals_the_three_forwards(shape, launches, act_quant, merged_calls):
    M, N = shape
    mods = [module(N, s, act_quant=act_quant) for s in range(3)]
    xi = activation(M, mods)
    assert (xi.row_off is not None) == bool(launches)
    got = harness.concurrent_linears(mods, xi)
    assert merged_calls == launches
    assert equal_lists(got, [m(xi) for m in mods]) and equal_lists(got, plain_reference(mods, xi))
    assert got[0].shape == (2, M // 2, N)
    if launches:     # no third copy of the weights: the modules' images are slices of the stacked operand
        run = mods[0].__dict__["_merged_run"]
        for i, m in enumerate(mods):
            assert m.offset_image(M, torch.float16)[0].data_ptr() == run.w[i * N].data_ptr()
        harness.concurrent_linears(mods, xi)
        assert merged_calls == launches * 2 and mods[0].__dict__["_merged_run"] is run      # ... built once


def test_weight_updates_reach_the_stacked_operand(merged_calls):
    M, N = BIG
    mods = [module(N, s) for s in range(3)]
    xi = activation(M, mods)
    before = harness.concurrent_linears(mods, xi)
    mods[1].weight.neg_().clamp_(min=-127)                  # in place: the version counter moves, the storage stays
    mods[2].weight = torch.roll(mods[2].weight, 1, 0)       # a new tensor
    mods[0].dequant_scale = torch.tensor(3e-4)              # a host scalar
    got = harness.concurrent_linears(mods, xi)
    assert merged_calls == [3, 3]
    assert equal_lists(got, plain_reference(mods, xi)) and equal_lists(got, [m(xi) for m in mods])
    assert not torch.equal(got[0], before[0]) and not torch.equal(got[1], before[1]) and not torch.equal(got[2], before[2])
    mods[1].load_state_dict({"weight": torch.roll(mods[1].weight, 3, 1), "dequant_scale": torch.tensor(2e-4)})
    got = harness.concurrent_linears(mods, xi)
    assert equal_lists(got, plain_reference(mods, xi))


def test_graph_capture_replays_equal_to_eager(merged_calls):
    M, N = BIG
    mods = [module(N, s) for s in range(3)]
    xi = activation(M, mods)
    eager = harness.concurrent_linears(mods, xi)             # (builds the stacked operand: a capture cannot)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr, stream=s):
        outs = harness.concurrent_linears(mods, xi)
    assert merged_calls == [3, 3]                            # the capture took the merged launch too
    for _ in range(2):
        for o in outs:
            o.zero_()
        gr.replay()
        torch.cuda.synchronize()
        assert equal_lists(outs, eager)


def test_run_lengths(merged_calls):
    M, N = BIG
    mods = [module(N, s) for s in range(3)] + [module(N2, s) for s in (3, 4)]
    xi = activation(M, mods)
    got = harness.concurrent_linears(mods, xi)
    assert merged_calls == [3, 2]                            # (N, N, N) and (N2, N2): two launches
    assert equal_lists(got, plain_reference(mods, xi))
    merged_calls.clear()
    six = [module(N, s) for s in range(6)]
    x6 = activation(M, six)
    got = harness.concurrent_linears(six, x6)
    assert merged_calls == [4, 2] and equal_lists(got, [m(x6) for m in six])


def test_modules_that_do_not_qualify_run_separately(merged_calls, monkeypatch):
    M, N = BIG
    mods = [module(N, s) for s in range(3)]
    xi = activation(M, mods)
    want = plain_reference(mods, xi)
    mods[1].offsets = False                                  # a module without an image
    assert equal_lists(harness.concurrent_linears(mods, xi), want) and merged_calls == []
    mods[1].offsets = True
    unequal = [mods[0], module(N2, 7), mods[2]]              # no two neighbours of one width
    xu = activation(M, unequal)
    assert equal_lists(harness.concurrent_linears(unequal, xu), plain_reference(unequal, xu)) and merged_calls == []
    mixed = [mods[0], module(N, 8, W8A8BFP32OFP32LinearWithQuantScale, "per-token")]      # a per-token consumer beside a per-tensor one
    assert harness._merge_key(mixed[0]) != harness._merge_key(mixed[1])
    assert equal_lists(harness.concurrent_linears(mods[:1], xi), want[:1]) and merged_calls == []      # a single module
    xf = (torch.randn(M, K, device=DEV) * 30).half()         # a float input: every module quantises for itself
    assert equal_lists(harness.concurrent_linears(mods, xf), [m(xf) for m in mods]) and merged_calls == []
    monkeypatch.setattr(harness, "merge_linears_enabled", False)                           # ASQ_MERGE_LINEARS=0
    assert equal_lists(harness.concurrent_linears(mods, xi), want) and merged_calls == []
    monkeypatch.setattr(harness, "merge_linears_enabled", True)
    assert equal_lists(harness.concurrent_linears(mods, xi), want) and merged_calls == [3]


def test_a_graph_captured_before_adoption_keeps_valid_buffers(merged_calls):
    """build_offset_image() at load, a capture before any eager merged call (captured as per-module launches on the modules' own buffers), then the eager
    merged call that moves the images into the stack: the earlier buffers are retired, not freed, and the graph still replays the same bits"""
    M, N = BIG
    mods = [module(N, s) for s in range(3)]
    assert all(m.build_offset_image() for m in mods)
    own = [m.offset_image(M, torch.float16) for m in mods]
    xi = activation(M, mods)
    want = plain_reference(mods, xi)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr, stream=s):
        outs = harness.concurrent_linears(mods, xi)
    assert merged_calls == []                               # nothing is adopted inside a capture
    assert equal_lists(harness.concurrent_linears(mods, xi), want) and merged_calls == [3]
    for m, old in zip(mods, own):
        assert m.offset_image(M, torch.float16)[0].data_ptr() != old[0].data_ptr()
        assert any(r[0] is old[0] and r[1] is old[1] for r in m.image.retired)
    del own
    junk = [torch.full((N, K), 77, dtype=torch.int8, device=DEV) for _ in range(6)]      # what freed buffers would be handed out for
    gr.replay()
    torch.cuda.synchronize()
    assert equal_lists(outs, want) and len(junk) == 6


def test_biased_modules_merge_and_their_bias_stays_one_tensor(merged_calls):
    M, N = BIG
    mods = [module(N, s, bias=True) for s in range(3)]
    xi = activation(M, mods)
    got = harness.concurrent_linears(mods, xi)
    assert merged_calls == [3] and equal_lists(got, plain_reference(mods, xi)) and equal_lists(got, [m(xi) for m in mods])
    run = mods[0].__dict__["_merged_run"]
    assert all(m.bias.data_ptr() == run.bias[i * N].data_ptr() and m.bias.shape == (N,) for i, m in enumerate(mods))      # the module's buffer IS the slice
    mods[0].bias.mul_(2.0)                                                        # in place
    mods[1].bias = torch.arange(N, dtype=torch.float32, device=DEV) * 1e-3        # a new tensor
    mods[2].load_state_dict({"weight": mods[2].weight.clone(), "bias": torch.ones(N), "dequant_scale": torch.tensor(1e-4)})
    got2 = harness.concurrent_linears(mods, xi)
    assert merged_calls == [3, 3] and equal_lists(got2, plain_reference(mods, xi))
    assert all(not torch.equal(a, b) for a, b in zip(got, got2))
    mixed = [mods[0], module(N, 9), mods[1]]                                      # a bias-free module between biased ones: no run
    xm = activation(M, mixed)
    assert equal_lists(harness.concurrent_linears(mixed, xm), plain_reference(mixed, xm)) and merged_calls == [3, 3]
