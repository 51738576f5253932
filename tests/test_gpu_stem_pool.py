"""halo_amd.norm.norm_relu_maxpool (halo_maxpool.hip) and halo_amd.hooks.fuse_norm_relu_pool on the device, against the restatement
of their numeric contract (tests/stem_pool_ref.py, which tests/test_stem_pool_host.py holds to torch's CPU autograd) and against
the stock chain on the same device.  The kernels run the chain's own operations with the chain's roundings and ATen's scan and
summation orders, so every comparison is bit for bit (NaN positions equal where the inputs carry NaN).

Backward against the stock device chain: a pixel in one or two windows has a sum of at most two terms, whose order cannot show; a
pixel at (odd, odd) lies in four windows.  Measured on the device: see test_backward_equals_the_stock_chain_on_the_device."""
import copy

import pytest
import torch
import torch.nn as nn

import norm_ref as N
import stem_pool_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
# The kernels' tile (halo_maxpool.hip): a lane owns 4 input columns and 4 output rows (forward) or 4 input row pairs (backward) on
# the 16-byte route, one output column (forward) / input column (backward) on the one-element route; 256 lanes per workgroup.
SHAPES = {
    "one_pixel": (1, 2, 1, 1),
    "one_row": (1, 2, 1, 9),
    "one_column": (1, 2, 9, 1),
    "tiny_even_odd": (1, 2, 2, 3),
    "odd_scalar": (2, 3, 5, 7),                 # odd both ways: the one-element route
    "even_vector": (1, 2, 8, 12),               # W % 4 == 0: the 16-byte route, one partial workgroup
    "unaligned_view": (1, 2, 8, 12),            # storage offset of one element: operands off 16 bytes
    "odd_rows_vector": (1, 3, 37, 52),          # odd rows, W a multiple of 4: a last strip of one output row and of one input row
    "ragged_columns": (1, 2, 6, 130),           # 65 / 130 one-element column groups per strip: a wave spans two strips
    "several_workgroups": (2, 5, 80, 160),      # 10 strips x 40 groups = 400 items per plane: two workgroups, the second partial
    # one row and one column more than a multiple of the tile: H = 65 = 8 strips of 8 input rows + 1, W = 260 = 65 groups of 4, one
    # more than a wave (the issue's 66 x 258 is for a 64 x 256 tile; this walk's tile is 8 rows x 4 columns per lane, 64 lanes per wave)
    "tile_plus_one": (1, 2, 65, 260),
    "tile_plus_one_scalar": (1, 2, 66, 258),    # the same on the one-element route (W % 4 != 0)
}


@pytest.fixture(autouse=True)
def every_size_served(monkeypatch):
    """the speed rule (the bits are the same on both sides) is switched off: these tests are about the kernels"""
    from halo_amd import norm
    monkeypatch.setattr(norm, "POOL_AUTOGRAD_MIN_ELEMENTS", 0)


def _on_device(t, unaligned):
    if not unaligned:
        return t.to(DEV)
    base = torch.empty(t.numel() + 1, device=DEV)
    base[1:].copy_(t.reshape(-1))
    out = base[1:].view(t.shape)
    assert out.is_contiguous() and out.data_ptr() % 16 == 4
    return out


@pytest.fixture(scope="module")
def cases():
    """per shape name: operands on the device, the restatement's results and the stock device chain's, computed once and left
    unchanged"""
    from halo_amd.dwconv import scale_shift
    out = {}
    for si, (name, shape) in enumerate(SHAPES.items()):
        bn = R.make_norm(shape[1], 7 + si)
        x, g = R.make_case(shape, 100 + si)
        scale, shift = (t.cpu() for t in scale_shift(copy.deepcopy(bn).to(DEV)))       # the device's rsqrt, not the host's
        ref = R.stem_pool_ref(x, scale, shift, g)
        # what the inputs must contain
        pre = bn(x)
        assert float(scale[0]) < 0 and (x.numel() < 30 or bool((pre == 0).any()))
        frac = float((g == 0).float().mean())
        assert bool((g == 0).any()) and (g.numel() < 1000 or 0.15 < frac < 0.25)          # a fifth of g is zero
        if x.numel() >= 30:
            assert bool(pre.isnan().any()) and bool(pre.isinf().any()) and bool(((x == 0) & x.signbit()).any())
        if R.planted(shape):
            tap, top = ref["tap"], ref["out"].shape[2] - 1
            assert int(tap[0, 0, 0, 0]) == R.BLOCKED                                   # a window without a positive tap
            assert int(tap[0, 1, 1, 1]) == 0 and float(pre[0, 1, 1, 1]) == float(pre[0, 1, 2, 2]) == float(ref["out"][0, 1, 1, 1]) > 0
            assert int(x[-1, -1, 2 * top, :2].isnan().sum()) == 2 and int(tap[-1, -1, top, 0]) == 5    # the last of two NaNs
        un = name == "unaligned_view"
        bn = bn.to(DEV)
        xd, gd = _on_device(x, un), _on_device(g, un)
        xs = xd.clone().requires_grad_(True)
        ys = nn.MaxPool2d(3, 2, 1)(torch.relu_(bn(xs)))
        (gxs,) = torch.autograd.grad(ys, xs, gd)
        out[name] = dict(bn=bn, x=xd, g=gd, ref=ref, scale=scale, y=ys.detach(), gx=gxs)
    assert any(R.planted(s) for s in SHAPES.values())
    return out


@pytest.mark.parametrize("name", list(SHAPES))
def test_forward_taps_and_backward_equal_the_restatement(cases, name):
    from halo_amd import _lib, norm
    c = cases[name]
    pool = nn.MaxPool2d(3, 2, 1)
    assert norm.pool_fallback_reason(c["x"], c["bn"], pool) is None
    x0 = c["x"].clone()
    x = c["x"].detach().requires_grad_(True)                     # the same storage and offset; the shared case stays as it is
    before = dict(norm.launches)
    y = norm.norm_relu_maxpool(x, c["bn"], pool)
    (tap, scale) = y.grad_fn.saved_tensors                       # the codes and scale, nothing else
    assert tap.dtype == torch.uint8 and tap.shape == y.shape and scale.shape == (x.shape[1],)
    (gx,) = torch.autograd.grad(y, [x], c["g"])
    for k in ("pool_fwd", "pool_bwd", "pool_taps"):              # one pass each way
        assert norm.launches[k] == before[k] + 1, k
    assert norm.launches["fwd"] == before["fwd"] and norm.launches["bwd"] == before["bwd"]
    assert N.same_bits(y.detach().cpu(), c["ref"]["out"]), "out against the restatement"
    assert N.same_bits(y.detach(), c["y"]), "out against the stock chain on the device"
    assert torch.equal(tap.cpu(), c["ref"]["tap"]), "tap codes"
    assert N.same_bits(gx.cpu(), c["ref"]["g_x"]), "g_x against the restatement"
    assert N.same_bits(c["x"], x0)                               # out of place
    # the C entry with the codes' pointer NULL writes the same output
    y2 = torch.empty_like(y)
    B, C, H, W = x.shape
    sc, sh = norm.cached_scale_shift(c["bn"])
    _lib.check(_lib.lib().halo_maxpool_affine_relu_fwd(_lib.ptr(c["x"]), _lib.ptr(sc), _lib.ptr(sh), _lib.ptr(y2), None, B, C, H, W,
                                                       _lib.stream_ptr(torch.device(DEV))))
    assert N.same_bits(y2, c["y"])


@pytest.mark.parametrize("name", list(SHAPES))
def test_backward_equals_the_stock_chain_on_the_device(cases, name):
    """Bit for bit at every pixel.  Only an (odd, odd) pixel, which lies in four windows, can see the order of a sum; were the
    library's pool backward to add in another order than ascending oh, ow, exactly those pixels would be held to the reassociation
    bound of a four-term float32 sum, |d| <= 3 * 2^-24 * |scale| * sum |g_i|, and any difference elsewhere would fail.  Measured on
    an MI355X with this suite's inputs: no pixel differs, so the bound is not needed and equality is asserted everywhere."""
    from halo_amd import norm
    c = cases[name]
    x = c["x"].detach().requires_grad_(True)
    y = norm.norm_relu_maxpool(x, c["bn"], nn.MaxPool2d(3, 2, 1))
    (gx,) = torch.autograd.grad(y, [x], c["g"])
    H, W = x.shape[2:]
    odd = (torch.arange(H, device=DEV) % 2 == 1).view(H, 1) & (torch.arange(W, device=DEV) % 2 == 1).view(1, W)
    a, b = torch.nan_to_num(gx, nan=7.0, posinf=8.0, neginf=-8.0), torch.nan_to_num(c["gx"], nan=7.0, posinf=8.0, neginf=-8.0)
    differs = a != b
    print("%s: pixels that differ from the stock device chain: %d at (odd, odd), %d elsewhere"
          % (name, int((differs & odd).sum()), int((differs & ~odd).sum())))
    assert not bool((differs & ~odd).any()), "a pixel in at most two windows differs"
    assert N.same_bits(gx, c["gx"]), "an (odd, odd) pixel differs"


def test_no_gradient_paths_keep_no_codes_and_launch_no_backward(cases):
    from halo_amd import norm
    c = cases["odd_rows_vector"]
    pool = nn.MaxPool2d(3, 2, 1)
    before = dict(norm.launches)
    with torch.no_grad():
        y = norm.norm_relu_maxpool(c["x"].clone().requires_grad_(True), c["bn"], pool)       # no_grad
    assert y.grad_fn is None and not y.requires_grad and N.same_bits(y, c["y"])
    y = norm.norm_relu_maxpool(c["x"], c["bn"], pool)                                         # an x that needs no gradient: the stem's image
    assert y.grad_fn is None and not y.requires_grad and N.same_bits(y, c["y"])
    w = torch.ones((), device=DEV, requires_grad=True)
    (y * w).sum().backward()                                                                  # a backward pass that reaches y
    assert norm.launches["pool_fwd"] == before["pool_fwd"] + 2
    assert norm.launches["pool_taps"] == before["pool_taps"] and norm.launches["pool_bwd"] == before["pool_bwd"]


def test_repeated_and_side_stream_calls_return_equal_bits(cases):
    from halo_amd.norm import norm_relu_maxpool
    c = cases["several_workgroups"]
    pool = nn.MaxPool2d(3, 2, 1)
    x = c["x"].clone().requires_grad_(True)
    runs = []
    for _ in range(2):
        y = norm_relu_maxpool(x, c["bn"], pool)
        runs.append((y.detach(),) + torch.autograd.grad(y, [x], c["g"]))
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        y = norm_relu_maxpool(x, c["bn"], pool)
        runs.append((y.detach(),) + torch.autograd.grad(y, [x], c["g"]))
    side.synchronize()
    for run in runs:
        assert N.same_bits(run[0], c["y"]) and N.same_bits(run[1], c["gx"])


def test_autograd_keeps_the_codes_and_not_the_rectified_tensor():
    """between forward and backward the operator holds out (4 bytes per pooled element) and the codes (1 byte); the parent's chain
    holds the rectified tensor (4 bytes per input element) and the pool's int64 indices (8 per pooled element) on top"""
    from halo_amd.norm import norm_relu_maxpool
    B, C, H, W = 2, 8, 160, 320
    bn = R.make_norm(C, 51).to(DEV)
    x = torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(52)).to(DEV).requires_grad_(True)
    norm_relu_maxpool(x, bn, nn.MaxPool2d(3, 2, 1))                     # scale and shift are cached now
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    y = norm_relu_maxpool(x, bn, nn.MaxPool2d(3, 2, 1))
    torch.cuda.synchronize()
    grown = torch.cuda.memory_allocated() - base
    pooled = B * C * (H // 2) * (W // 2)
    print("held after the forward: %d bytes; out + codes: %d" % (grown, 5 * pooled))
    assert y.requires_grad and 4 * pooled <= grown <= 4 * pooled + pooled + (1 << 20)


@pytest.fixture
def deterministic_convolutions(monkeypatch):
    """the library's deterministic convolution algorithms, as tests/test_gpu_norm_relu.py asks for them: two runs of the unhooked
    model then agree bit for bit, and so must the hooked one"""
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)


@pytest.mark.parametrize("others", [False, True], ids=["alone", "with_the_block_and_pair_hooks"])
def test_hooked_backbone_equals_the_unhooked_one(deterministic_convolutions, monkeypatch, others):
    from halo_amd import hooks, norm
    monkeypatch.setattr(norm, "AUTOGRAD_MIN_ELEMENTS", {"plain": 0, "affine": 0})
    torch.manual_seed(41)
    plain = N.randomize_norms(N.backbone(), 42).to(DEV)
    if others:
        hooked, pairs = N.hooked_copy(plain)                     # use_fused_frozen_norm on the blocks, fuse_norm_relu_pairs on the stem
        assert pairs == 1
    else:
        hooked = copy.deepcopy(plain)
    assert hooks.fuse_norm_relu_pool(hooked) == 1 and hooks.fuse_norm_relu_pairs(hooked) == 0
    x = torch.randn(2, 3, 33, 47).to(DEV)
    g_of = lambda outs: [torch.randn(o.shape, generator=torch.Generator().manual_seed(31 + i)).to(DEV) for i, o in enumerate(outs)]
    o1, g1 = N.run_with_grads(plain, x, g_of)
    before = dict(norm.launches)
    oh, gh = N.run_with_grads(hooked, x, g_of)
    assert len(o1) == len(oh) and all(torch.equal(a, b) for a, b in zip(o1, oh)), "forward"
    for k, (a, h) in enumerate(zip(g1, gh)):
        assert torch.equal(a, h), "gradient %d" % k
    assert norm.launches["pool_fwd"] == before["pool_fwd"] + 1 and norm.launches["pool_bwd"] == before["pool_bwd"] + 1     # the stem
    blocks = 9 if others else 0                                                                # 3 x 3 norms of the blocks, not the stem
    assert norm.launches["fwd"] == before["fwd"] + blocks and norm.launches["bwd"] == before["bwd"] + blocks


def test_speed_rule_hands_small_tensors_that_need_a_gradient_to_the_pair(cases, monkeypatch):
    from halo_amd import norm
    c = cases["several_workgroups"]
    pool = nn.MaxPool2d(3, 2, 1)
    monkeypatch.setattr(norm, "POOL_AUTOGRAD_MIN_ELEMENTS", c["x"].numel() + 1)
    monkeypatch.setattr(norm, "AUTOGRAD_MIN_ELEMENTS", {"plain": 0, "affine": 0})
    x = c["x"].clone().requires_grad_(True)
    before = dict(norm.launches)
    y = norm.norm_relu_maxpool(x, c["bn"], pool)                          # norm_relu's pass, then the library's pool
    (gx,) = torch.autograd.grad(y, [x], c["g"])
    assert norm.launches["pool_fwd"] == before["pool_fwd"] and norm.launches["fwd"] == before["fwd"] + 1
    assert N.same_bits(y.detach(), c["y"]) and N.same_bits(gx, c["gx"])
    with torch.no_grad():                                                 # without a gradient the rule turns nothing away
        assert N.same_bits(norm.norm_relu_maxpool(x, c["bn"], pool), c["y"])
    assert norm.launches["pool_fwd"] == before["pool_fwd"] + 1
