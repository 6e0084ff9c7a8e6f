"""ops.aggregate_gru (csrc/mp_gru.h) against the float64 reference of aggregate_gru_ref.py: real values within
the derived bound over one-axis sweeps (fp32 carries the layout check), the second cell of a stack, same bits,
and gradients against float64 autograd."""
import numpy as np
import pytest
import torch

from aggregate_gru_ref import gru_ref, segment_sum

pytestmark = pytest.mark.gpu

DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
UNIT = {"f32": 0.0, "bf16": 2.0 ** -8, "f16": 2.0 ** -11}       # unit roundoff of a narrowing
U24 = 2.0 ** -24
ACT = 4 * U24                                                    # kGruActUlps of mp_gru.h
HUB = [0, 1, 300, 0, 0, 1, 5, 16, 17, 0, 33, 2, 0]              # segment lengths of the seg_ptr case

BASE = dict(dt="f32", op="add", d=64, u=64, count=10, size=65, gather="int32", lens=None, out="f32", off=0,
            bias="f32")
# one-axis sweeps around BASE; the plan boundaries are those of GruMakePlan (mp_gru.h)
CASES = {
    "base": {}, "bf16": dict(dt="bf16"), "f16": dict(dt="f16"), "mean": dict(op="mean"), "mean-bf16": dict(op="mean", dt="bf16"),
    **{"d%d" % d: dict(d=d) for d in (1, 7, 8, 31, 32, 33, 128, 129)},
    **{"U%d" % u: dict(u=u) for u in (1, 15, 16, 17, 31, 32, 33, 64, 65, 128, 129, 256)},
    "second-cell": dict(gather=None, count=1), "second-cell-bf16": dict(gather=None, count=1, dt="bf16", out="same"),
    **{"size%d" % s: dict(size=s) for s in (0, 1, 15, 16, 17, 257)},
    **{"count%d" % c: dict(count=c) for c in (1, 3, 17)},
    "seg": dict(lens=HUB), "seg-bf16-mean": dict(lens=HUB, dt="bf16", op="mean"),
    "gather-none": dict(gather=None), "gather-int32-bad": dict(gather="int32-bad"), "gather-int64-bad": dict(gather="int64-bad"),
    "off4": dict(off=1), "off2-bf16": dict(off=1, dt="bf16"),
    "no-bias": dict(bias=None), "bias-same-f16": dict(bias="same", dt="f16"),
    "out-bf16": dict(dt="bf16", out="same"), "out-f16": dict(dt="f16", out="same"),
    # CH 4 | 8 at max(d, U) = 128 | 129; 16 bits, CH 4 (NT 4): c passes 1 | 2 at U 64 | 65; CH 8 (NT 2): r passes
    # 2 | 3 | 4 at U 128 | 129, 192 | 193, c passes 5 | 6 at 160 | 161; packed columns at d = U = 128
    "bf16-d128-U128": dict(dt="bf16", d=128, u=128), "bf16-d129-U128": dict(dt="bf16", d=129, u=128, size=33),
    "bf16-d256-U192": dict(dt="bf16", d=256, u=192, size=17), "bf16-d256-U193": dict(dt="bf16", d=256, u=193, size=17),
    "f16-d8-U160": dict(dt="f16", d=8, u=160, size=17), "f16-d8-U161": dict(dt="f16", d=8, u=161, size=17),
    # fp32, CH 4 (NT 2): r passes 1 | 2 at U 64 | 65, c passes 1 | 2 at 32 | 33 (above); CH 8 (NT 1): one r pass per 32
    # and one c pass per 16 columns
    "f32-d128-U128": dict(d=128, u=128), "f32-d256-U256": dict(d=256, u=256, size=17, count=3),
    "f32-d200-U144": dict(d=200, u=144, size=17), "f32-d200-U145": dict(d=200, u=145, size=17),
    # past the launcher's grid cap: 512 workgroups x 8 runs x 16 destinations
    "grid-cap": dict(dt="bf16", d=8, u=16, count=1, size=65536 + 17),
}


def make(case, seed=0):
    """-> (positional args, keyword args for ops.aggregate_gru on the device, args for gru_ref)"""
    c = dict(BASE, **case)
    rng = np.random.default_rng(seed)
    d, u, dt = c["d"], c["u"], DT[c["dt"]]
    seg = np.arange(c["size"] + 1) * c["count"] if c["lens"] is None else np.concatenate([[0], np.cumsum(c["lens"])])
    size, e = len(seg) - 1, int(seg[-1])
    rows = max(e, 1) if c["gather"] is None else 97
    flat = torch.zeros(rows * d + 8, dtype=dt)
    flat[c["off"]:c["off"] + rows * d] = torch.as_tensor(rng.standard_normal(rows * d), dtype=dt)
    table = flat.cuda()[c["off"]:c["off"] + rows * d].view(rows, d)
    dev = lambda a, t=dt: torch.as_tensor(a, dtype=t).cuda()
    state = dev(rng.standard_normal((size, u)))
    wg, wc = dev(rng.standard_normal((d + u, 2 * u)) / np.sqrt(d + u)), dev(rng.standard_normal((d + u, u)) / np.sqrt(d + u))
    bt = torch.float32 if c["bias"] == "f32" else dt
    bg, bc = (None, None) if c["bias"] is None else (dev(1 + rng.standard_normal(2 * u), bt), dev(rng.standard_normal(u), bt))
    gi = None
    if c["gather"] is not None:
        gi = rng.integers(0, rows, e).astype(np.int64 if c["gather"].startswith("int64") else np.int32)
        if c["gather"].endswith("bad"):
            bad = [-1, rows] + ([2 ** 40, 2 ** 32 + 3] if gi.dtype == np.int64 else [])
            gi[::3] = np.resize(bad, len(gi[::3]))
    kw = dict(gate_bias=bg, cand_bias=bc, out_dtype=torch.float32 if c["out"] == "f32" else None)
    kw.update(dict(count=c["count"]) if c["lens"] is None else dict(seg_ptr=torch.as_tensor(seg).cuda()))
    stored = lambda t: None if t is None else t.double().cpu().numpy()
    return ((c["op"], table, None if gi is None else torch.as_tensor(gi).cuda(), size, state, wg, wc), kw,
            (c["op"], stored(table), gi, seg, stored(state), stored(wg), stored(wc), stored(bg), stored(bc), dt))


def bound(c, ref_args, parts, out_unit):
    """The error of every pre-activation is that of test_real_values_within_bound of the dense test: (K + 2) 2^-24
    sum |a||w|, x4 (an MFMA's rounding is not documented), and the operand errors times |w| - for m the fold's
    (len + 1) 2^-24 sum |x| (mean: + 3 x 2^-24) and one narrowing unit; for r * h the error of r times |h|, one fp32
    multiply and one narrowing unit.  sigmoid has slope <= 1/4 and tanh <= 1, each evaluated within ACT; the blend
    moves by |h - c| du + (1 - u) dc and rounds four times on values below |h| + |c|; then the output's own rounding."""
    op, table, gi, seg, h, wg, wc, bg, bc, _ = ref_args
    d, u_dim, unit = c["d"], c["u"], UNIT[c["dt"]]
    m, r, u, cc, rh = (np.abs(parts[k]) for k in ("m", "r", "u", "c", "rh"))
    longest = int(np.diff(seg).max()) if len(seg) > 1 else 0
    dm = ((longest + 1 + (3 if op == "mean" else 0)) * U24) * segment_sum(op, np.abs(table), gi, seg) + unit * m
    acc = 4 * (d + u_dim + 2) * U24
    e_g = acc * (np.concatenate([m, np.abs(h)], 1) @ np.abs(wg) + (0 if bg is None else np.abs(bg))) + dm @ np.abs(wg[:d])
    dr, du = e_g[:, :u_dim] / 4 + ACT, e_g[:, u_dim:] / 4 + ACT
    drh = dr * np.abs(h) + (U24 + unit) * rh
    e_c = (acc * (np.concatenate([m, rh], 1) @ np.abs(wc) + (0 if bc is None else np.abs(bc))) + dm @ np.abs(wc[:d])
           + drh @ np.abs(wc[d:]))
    out_mag = np.abs(h) + cc
    return np.abs(h - parts["c"]) * du + (1 - parts["u"]) * (e_c + ACT) + (4 * U24 + out_unit) * out_mag


@pytest.mark.parametrize("name", sorted(CASES))
def test_real_values_within_bound(name):
    from euler_amd import ops
    c = dict(BASE, **CASES[name])
    args, kw, ref_args = make(CASES[name], seed=1)
    out = ops.aggregate_gru(*args, **kw)
    assert out.shape == (args[3], c["u"]) and out.dtype == (kw["out_dtype"] or args[1].dtype)
    want, parts = gru_ref(*ref_args)
    ratio = np.abs(out.double().cpu().numpy() - want) / bound(c, ref_args, parts, 0.0 if c["out"] == "f32" else UNIT[c["dt"]])
    print(name, "largest error / bound: %.3f" % (ratio.max() if ratio.size else 0.0))
    assert np.all(ratio <= 1.0)


@pytest.mark.parametrize("dt", sorted(DT))
def test_second_cell_and_same_bits(dt):
    """gather_indices=None, count=1 is the cell applied to the rows themselves (the second cell of a stack): the bits
    of the same call with the identity written out as indices; count and the equivalent seg_ptr, a second run and a
    second stream give the same bits"""
    from euler_amd import ops
    same = lambda a, b: torch.equal(a.view(torch.int16 if a.element_size() == 2 else torch.int32),
                                    b.view(torch.int16 if b.element_size() == 2 else torch.int32))
    args, kw, _ = make(dict(dt=dt, gather=None, count=1, out="same"), seed=2)
    ident = torch.arange(args[3], dtype=torch.int32, device="cuda")
    assert same(ops.aggregate_gru(*args, **kw), ops.aggregate_gru(args[0], args[1], ident, *args[3:], **kw))
    args, kw, _ = make(dict(dt=dt), seed=2)
    first = ops.aggregate_gru(*args, **kw)
    seg = torch.arange(BASE["size"] + 1, device="cuda") * BASE["count"]
    as_seg = ops.aggregate_gru(*args, **dict({k: v for k, v in kw.items() if k != "count"}, seg_ptr=seg))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = ops.aggregate_gru(*args, **kw)
    side.synchronize()
    for t in (ops.aggregate_gru(*args, **kw), as_seg, other):
        assert same(first, t)


def cell64(m, h, wg, wc, bg, bc, dt, mag=False):
    """the cell in float64 torch, for autograd; mag: its magnitude graph - absolute operands, every activation
    replaced by a line of its largest slope and every difference by a sum, so that its gradient bounds the sum
    of the absolute terms of the true one"""
    sig = (lambda z: 0.5 + z / 4) if mag else torch.sigmoid
    u_dim = h.shape[1]
    zg = torch.cat([m, h], 1) @ wg + bg
    r, u = sig(zg[:, :u_dim]), sig(zg[:, u_dim:])
    rh = r * h
    if not mag:
        rh = rh + (rh.detach().to(dt).double() - rh.detach())
    zc = torch.cat([m, rh], 1) @ wc + bc
    return u * h + (1 + u) * zc if mag else u * h + (1 - u) * torch.tanh(zc)


@pytest.mark.parametrize("dt", sorted(DT))
def test_gradients(dt, monkeypatch):
    """The device's gradients against float64 autograd of the reference on the stored values.  Bound of an element, as
    in the dense test: the magnitude graph's gradient times (terms + 2) 2^-24, x4, terms = e + d + 3 U; 16-bit
    storage adds three narrowing units (m, r * h, and the returned gradient itself)."""
    from euler_amd import ops
    count, size, d, u, rows = 4, 37, 24, 20, 50
    monkeypatch.setattr(ops, "POOL_GRAD_CHUNK_ROWS", 10 * count)      # 37 destinations: four chunks
    rng = np.random.default_rng(3)
    gi = rng.integers(0, rows, size * count)
    gi[5], gi[17] = -1, 2 ** 40
    shapes = dict(table=(rows, d), state=(size, u), wg=(d + u, 2 * u), wc=(d + u, u), bg=(2 * u,), bc=(u,))
    dev = {k: torch.tensor(rng.standard_normal(s) / (np.sqrt(d + u) if k[0] == "w" else 1.0), dtype=DT[dt],
                           device="cuda", requires_grad=True) for k, s in shapes.items()}
    g_out = rng.standard_normal((size, u))
    out = ops.aggregate_gru("add", dev["table"], torch.as_tensor(gi).cuda(), size, dev["state"], dev["wg"], dev["wc"],
                            dev["bg"], dev["bc"], count=count, out_dtype=torch.float32)
    out.backward(torch.tensor(g_out, dtype=torch.float32, device="cuda"))
    ok = torch.as_tensor((gi >= 0) & (gi < rows))
    idx = torch.as_tensor(np.where(ok, gi, 0))
    grads = []
    for mag in (False, True):
        cpu = {k: (v.detach().double().cpu().abs() if mag else v.detach().double().cpu()).requires_grad_() for k, v in dev.items()}
        m = (cpu["table"][idx] * ok[:, None]).view(size, count, d).sum(1)
        if not mag:
            m = m + (m.detach().to(DT[dt]).double() - m.detach())
        res = cell64(m, cpu["state"], cpu["wg"], cpu["wc"], cpu["bg"], cpu["bc"], DT[dt], mag)
        res.backward(torch.tensor(np.abs(g_out) if mag else g_out))
        grads.append({k: v.grad for k, v in cpu.items()})
    tol = 4 * (size * count + d + 3 * u + 2) * U24 + 3 * UNIT[dt]
    for k in shapes:
        assert torch.all((dev[k].grad.double().cpu() - grads[0][k]).abs() <= tol * grads[1][k]), k
