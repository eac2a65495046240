"""hc_conv_rows_fused_bwd (csrc/conv_rows.hip, mode 2): the row-unit data gradient that forms dy3 / dy1 / dx_id of an identity
RepBlock in its own prologue, against the two launches it replaces - hc_rep_bwd_apply_z followed by the data gradient of
hc_conv_small - on the same inputs.  Both compile the same fma chains (csrc/rep_ew.h) and the same k-loop, so every comparison is
``torch.equal``: there is no tolerance.

Inputs: random bf16 x, y3 / y1 from the block's own forward convolutions, coef / bcoef from the real finalize kernels (the ReLU mask has
both signs), random g.  Shapes: the smallest that reach every path of the kernel - the two tuned instantiations (192 @ 14 x 14 with two
units per image, 96 @ 28 x 28 with four, so that a team walks two) and the family form of both channel counts with a ragged last unit
and discarded columns."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

EPS = 1e-5
# (C, N, H, W)
SHAPES = [(192, 3, 14, 14), (192, 2, 9, 12), (96, 2, 28, 28), (96, 1, 10, 20)]
_CACHE = {}


def _inputs(ch, N, H, W, act, frozen):
    """Everything both paths read, computed once per case: (st, geom, w3, w1, g, coef, y3, y1, x, bcoef) and the reference
    (dy3, dy1, dx_id, dx) of the two launches."""
    key = (ch, N, H, W, act, frozen)
    if key in _CACHE:
        return _CACHE[key]
    from holocron_amd import _lib
    from holocron_amd._lib import RepBnBwdDesc, RepBnDesc, check, ptr, stream
    from holocron_amd.nn import repblock_op as rb
    from holocron_amd.ops import conv as cv
    dev = torch.device("cuda:0")
    lib = _lib.load()
    gen = torch.Generator().manual_seed(4100 + ch + 7 * H + W + act + 2 * frozen)
    shape = (N, ch, H, W)
    x = cv.to_cl_bf16((torch.randn(shape, generator=gen) * 0.8 + 0.1).to(dev))
    g = cv.to_cl_bf16(torch.randn(shape, generator=gen).to(dev))
    w3 = (torch.randn((ch, ch, 3, 3), generator=gen) * (2.0 / (ch * 9)) ** 0.5).to(dev)
    w1 = (torch.randn((ch, ch, 1, 1), generator=gen) * (2.0 / ch) ** 0.5).to(dev)
    st = rb.RepState(1, True)
    geom = (N, ch, H, W, ch)
    R = _lib.stat_replicas()
    stats = torch.zeros((2, R, 2, ch), dtype=torch.float32, device=dev)
    y3, y1 = rb.block_convs_forward(st, x, w3, w1, geom, stats)
    xs = torch.zeros((R, 2, ch), dtype=torch.float32, device=dev)
    npix = N * H * W
    check(lib.hc_channel_stats(ptr(x), ptr(xs), npix, ch, stream()), "hc_channel_stats")
    gam = [(torch.rand(ch, generator=gen) + 0.5).to(dev) for _ in range(3)]
    bet = [(torch.randn(ch, generator=gen) * 0.3).to(dev) for _ in range(3)]
    rm = [(torch.randn(ch, generator=gen) * 0.1).to(dev) for _ in range(3)]
    rv = [(torch.rand(ch, generator=gen) + 0.5).to(dev) for _ in range(3)]
    nbt = [torch.zeros((), dtype=torch.int64, device=dev) for _ in range(3)]
    coef = torch.empty((4, ch), dtype=torch.float32, device=dev)
    save = torch.empty((6, ch), dtype=torch.float32, device=dev)
    d = RepBnDesc()
    for b, s in enumerate((stats[0], stats[1], xs)):
        d.gamma[b], d.beta[b], d.running_mean[b], d.running_var[b] = ptr(gam[b]), ptr(bet[b]), ptr(rm[b]), ptr(rv[b])
        d.num_batches_tracked[b] = ptr(nbt[b])
        d.stats[b] = None if frozen else ptr(s)
    d.coef, d.save, d.C, d.count, d.eps, d.momentum, d.training = ptr(coef), ptr(save), ch, npix, EPS, 0.1, 0 if frozen else 1
    check(lib.hc_rep_bn_finalize(C.byref(d), stream()), "hc_rep_bn_finalize")
    red = torch.zeros((R, 4, ch), dtype=torch.float32, device=dev)
    check(lib.hc_rep_bwd_reduce_z(ptr(g), ptr(coef), act, ptr(y3), ptr(y1), ptr(x), ptr(red), npix, ch, stream()), "hc_rep_bwd_reduce_z")
    dgam = torch.empty((3, ch), dtype=torch.float32, device=dev)
    dbet = torch.empty((3, ch), dtype=torch.float32, device=dev)
    bcoef = torch.empty((9, ch), dtype=torch.float32, device=dev)
    bd = RepBnBwdDesc()
    bd.red, bd.save, bd.bcoef = ptr(red), ptr(save), ptr(bcoef)
    for b in range(3):
        bd.gamma[b], bd.dgamma[b], bd.dbeta[b] = ptr(gam[b]), ptr(dgam[b]), ptr(dbet[b])
    bd.C, bd.count, bd.has_identity, bd.accumulate, bd.frozen = ch, npix, 1, 0, 1 if frozen else 0
    check(lib.hc_rep_bn_bwd_finalize(C.byref(bd), stream()), "hc_rep_bn_bwd_finalize")
    # the reference: the two launches
    dy3, dy1, dxid = torch.empty_like(y3), torch.empty_like(y1), torch.empty_like(x)
    check(lib.hc_rep_bwd_apply_z(ptr(g), ptr(coef), act, ptr(y3), ptr(y1), ptr(x), ptr(bcoef), ptr(dy3), ptr(dy1), ptr(dxid), npix, ch,
                                 stream()), "hc_rep_bwd_apply_z")
    dx = rb.block_dgrad(st, dy3, dy1, dxid, w3, w1, geom)
    torch.cuda.synchronize()
    if act == 1:      # the ReLU mask has both signs
        z = coef[0].view(1, -1, 1, 1) * y3.float() + coef[1].view(1, -1, 1, 1) * y1.float() + coef[2].view(1, -1, 1, 1) * x.float() + coef[3].view(1, -1, 1, 1)
        pos = float((z > 0).float().mean())
        assert 0.1 < pos < 0.9, pos
    _CACHE[key] = (st, geom, w3, w1, g, coef, y3, y1, x, bcoef, (dy3, dy1, dxid, dx))
    return _CACHE[key]


def _run_fused(inp, act, poison=False):
    from holocron_amd.nn import repblock_op as rb
    st, geom, w3, w1, g, coef, y3, y1, x, bcoef, _ = inp
    sdg = rb.fused_dgrad_desc(st, geom)
    assert sdg is not None, "hc_conv_rows_fused_bwd must take %r" % (geom,)
    # poison: the same launch into buffers full of NaN - a read of dy1 / dx_id that does not see the kernel's own stores shows up in dx
    bufs = tuple(torch.full_like(x, float("nan")) for _ in range(4)) if poison else None
    out = rb.block_dgrad_fused(st, sdg, g, coef, act, y3, y1, x, bcoef, w3, w1, bufs=bufs)
    torch.cuda.synchronize()
    return out


def _compare(got, ref, what):
    for name, a, b in zip(("dy3", "dy1", "dx_id", "dx"), got, ref):
        assert not bool(torch.isnan(a.float()).any()), (what, name, "NaN")
        same = torch.equal(a, b)
        if not same:
            diff = (a.float() - b.float()).abs()
            nz = diff.nonzero()
            print(what, name, "differs in", int((diff > 0).sum()), "of", a.numel(), "first (n, c, h, w):", nz[0].tolist(), "max", float(diff.max()))
        assert same, (what, name)


CASES = [(s, act, 0) for s in SHAPES for act in (0, 1)] + [(SHAPES[1], 1, 1)]


@pytest.mark.parametrize("shape,act,frozen", CASES, ids=["%d_n%d_%dx%d_act%d_frozen%d" % (s + (a, f)) for s, a, f in CASES])
def test_fused_launch_equals_the_two_launches(shape, act, frozen):
    inp = _inputs(*shape, act, frozen)
    _compare(_run_fused(inp, act), inp[-1], (shape, act, frozen))


def test_fused_launch_reads_back_its_own_stores():
    """dy1 (re-staged after the ninth tap) and dx_id (the epilogue's residual) are written and read back by the same launch: with both
    buffers full of NaN beforehand a stale read poisons dx."""
    shape, act = SHAPES[2], 1
    inp = _inputs(*shape, act, 0)
    _compare(_run_fused(inp, act, poison=True), inp[-1], (shape, "poisoned"))


def test_repblock_step_is_bit_equal_with_the_switch_on_and_off(monkeypatch):
    """One 192-channel RepBlock, N = 4, 14 x 14: forward + backward with the fused launch and with the two launches
    (HC_REP_FUSED_BWD, mirrored by repblock_op.FUSED_BWD): dx and both weight gradients are the same bits."""
    import holocron_amd as h
    from holocron_amd.nn import repblock_op as rb
    from holocron_amd.ops import conv as cv
    dev = torch.device("cuda:0")
    torch.manual_seed(11)
    blk = h.models.classification.repvgg.RepBlock(192, 192, 1, True).to(dev).train()
    x0 = cv.to_cl_bf16(torch.randn(4, 192, 14, 14, device=dev))
    up = cv.to_cl_bf16(torch.randn(4, 192, 14, 14, device=dev))
    state = {k: v.clone() for k, v in blk.state_dict().items()}
    res = []
    for on in (True, False):
        monkeypatch.setattr(rb, "FUSED_BWD", on)
        blk.load_state_dict(state)
        blk.zero_grad(set_to_none=True)
        x = x0.clone().requires_grad_(True)
        prof, cv.PROFILE = cv.PROFILE, []
        try:
            blk(x).backward(up)
            torch.cuda.synchronize()
            fams = [e[0] for e in cv.PROFILE]
        finally:
            cv.PROFILE = prof
        # with the switch on the pair (bn_elementwise apply + conv_rows data gradient) is one conv_rows entry
        res.append((x.grad.clone(), blk.branches[0][0].weight.grad.clone(), blk.branches[1][0].weight.grad.clone(), fams))
    (dx_a, dw3_a, dw1_a, fam_a), (dx_b, dw3_b, dw1_b, fam_b) = res
    assert fam_a.count("bn_elementwise") + 1 == fam_b.count("bn_elementwise") and fam_a.count("conv_rows") == fam_b.count("conv_rows"), (fam_a, fam_b)
    assert torch.equal(dx_a, dx_b) and torch.equal(dw3_a, dw3_b) and torch.equal(dw1_a, dw1_b)
