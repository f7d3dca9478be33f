"""GPU: the attention kernels (csrc/attention.hip) through the C ABI against the float64 reference, ELEMENT BY ELEMENT.

omnipq_attn_fwd / omnipq_attn_bwd / omnipq_attn_dropout_mask are called directly, on buffers this module lays out itself, so
that lse2, delta and every stride are under the test's control.  Every element of O, lse2, delta, dQ, dK and dV must be
inside the bound tests/attention_reference.py derives from the kernels' roundings (no exceptions, no norms); output
buffers are filled with a NaN pattern beforehand, and whatever the layout leaves between the rows must still hold it
afterwards.  The cases are attention_reference.CASES -- the CPU suite holds an emulation of the kernels' arithmetic, and
seven mutants of it, against the same bounds on the same cases (tests/test_attention_reference.py).

Each test prints the largest error / bound ratio per output (`RATIO <library> <case>: O=... lse2=...`, pytest -s).
NOT YET MEASURED: this module has not run on an MI355X (no GPU could be had while it was written); the table of the
largest ratios per library and output belongs here after its first run.  On the CPU emulation the four e16 outputs stay
at or below 1 / 1.5 of their bounds on every case.
"""
import ctypes

import pytest
import torch

from conftest import REPO  # noqa: F401  (sys.path set-up)
import attention_reference as ar

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64          # elements in front of and behind every output buffer
NAN16 = {torch.bfloat16: 0x7FC1, torch.float16: 0x7E01}       # a NaN of each element type, as the int16 it is stored as
SEED, SALT = 0x1234567887654321, 5


def lib_of(dtype):
    import sa_fused
    ext = sa_fused._ext
    if dtype is torch.float16 and ext.LIB_F16_PATH is None:
        pytest.skip("no IEEE-half library in this build")
    return ext._LIBS[dtype], ext


class Slot:
    """One (T, N, E) tensor inside a flat e16 buffer: element (t, n, e) at buf[GUARD + off + t * tok + n * bat + e].  Slots
    of one layout may share a buffer (q|k|v side by side)."""

    def __init__(self, buf, off, tok, bat, T, N, E):
        assert off % 4 == 0 and tok % 4 == 0 and bat % 4 == 0 and tok >= 0
        assert GUARD + off + (T - 1) * tok + (N - 1) * bat + E <= buf.numel() - GUARD, "slot outside its buffer"
        self.buf, self.off, self.tok, self.bat, self.shape = buf, GUARD + off, tok, bat, (T, N, E)

    def view(self, buf=None):
        return (self.buf if buf is None else buf).as_strided(self.shape, (self.tok, self.bat, 1), self.off)

    def ptr(self):
        return ctypes.c_void_p(self.buf.data_ptr() + 2 * self.off)

    def put(self, x_bhtd, N, H):                       # (B, T, D) head-major -> the slot
        B, T, D = x_bhtd.shape
        self.view().copy_(x_bhtd.reshape(N, H, T, D).permute(2, 0, 1, 3).reshape(T, N, H * D).to(DEV))

    def get(self, N, H):                               # the slot -> (B, T, D) on the CPU
        T, _, E = self.shape
        return self.view().reshape(T, N, H, E // H).permute(1, 2, 0, 3).reshape(N * H, T, E // H).cpu()


def new_buf(numel, dtype):
    buf = torch.empty(numel + 2 * GUARD, dtype=dtype, device=DEV)
    buf.view(torch.int16).fill_(NAN16[dtype])
    return buf


def untouched(slots):
    """every element of the slots' buffers that belongs to no slot still holds the fill pattern"""
    seen = {}
    for s in slots:
        key = s.buf.data_ptr()
        if key not in seen:
            seen[key] = (s.buf, torch.zeros(s.buf.numel(), dtype=torch.bool, device=DEV))
        s.view(seen[key][1]).fill_(True)
    for buf, owned in seen.values():
        if not bool((buf.view(torch.int16)[~owned] == NAN16[buf.dtype]).all()):
            return False
    return True


def layout(case):
    """-> {q, k, v, o, do, dq, dk, dv: Slot}.  Inputs are written into NaN-filled buffers too: a kernel that reads between
    the rows of a padded layout poisons its result."""
    L, S, N, E, dt, lay = case["L"], case["S"], case["N"], case["H"] * case["D"], case["dtype"], case["layout"]

    def plain(T, pitch=None, batch_major=False):
        pitch = E if pitch is None else pitch
        buf = new_buf(T * N * pitch, dt)
        return Slot(buf, 0, pitch, T * pitch, T, N, E) if batch_major else Slot(buf, 0, N * pitch, pitch, T, N, E)

    if lay in ("contig", "pitch4"):
        pitch = E if lay == "contig" else E + 4
        names = dict(q=L, k=S, v=S, o=L, do=L, dq=L, dk=S, dv=S)
        return {n: plain(T, pitch) for n, T in names.items()}
    if lay == "own":
        return dict(q=plain(L), k=plain(S, E + 4), v=plain(S, batch_major=True), o=plain(L, E + 8), do=plain(L, E + 8),
                    dq=plain(L, E + 4, batch_major=True), dk=plain(S, E + 12), dv=plain(S, E + 8, batch_major=True))
    out = dict(o=plain(L, batch_major=True), do=plain(L, batch_major=True))
    if lay == "self":
        assert L == S
        for names in (("q", "k", "v"), ("dq", "dk", "dv")):
            buf = new_buf(N * L * 3 * E, dt)
            for i, n in enumerate(names):
                out[n] = Slot(buf, i * E, 3 * E, L * 3 * E, L, N, E)
        return out
    assert lay == "cross"
    out["q"], out["dq"] = plain(L, batch_major=True), plain(L, batch_major=True)
    for names in (("k", "v"), ("dk", "dv")):
        buf = new_buf(N * S * 2 * E, dt)
        for i, n in enumerate(names):
            out[n] = Slot(buf, i * E, 2 * E, S * 2 * E, S, N, E)
    return out


def f32_out(rows, cols):
    buf = torch.full((rows * cols + 2 * GUARD,), float("nan"), device=DEV)
    return buf, ctypes.c_void_p(buf.data_ptr() + 4 * GUARD)


def f32_get(buf, rows, cols):
    guards = torch.cat([buf[:GUARD], buf[GUARD + rows * cols:]])
    assert bool(torch.isnan(guards).all()), "wrote outside lse2 / delta"
    return buf[GUARD:GUARD + rows * cols].reshape(rows, cols).cpu()


def ll(*vals):
    return (ctypes.c_longlong * len(vals))(*vals)


def run_kernels(case, q, k, v, do):
    """-> got {output: CPU tensor}, keep mask (B, L, S) or None"""
    lib, ext = lib_of(case["dtype"])
    L, S, N, H, D, p = (case[n] for n in ("L", "S", "N", "H", "D", "p"))
    B = N * H
    sl = layout(case)
    for name, x in (("q", q), ("k", k), ("v", v), ("do", do)):
        sl[name].put(x, N, H)
    strides = ll(*(x for n in ("q", "k", "v", "o") for x in (sl[n].tok, sl[n].bat)))
    gstrides = ll(*(x for n in ("dq", "dk", "dv") for x in (sl[n].tok, sl[n].bat)))
    assert (sl["do"].tok, sl["do"].bat) == (sl["o"].tok, sl["o"].bat)
    seed = torch.tensor([SEED], dtype=torch.int64, device=DEV) if p > 0 else None
    seed_p = ctypes.c_void_p(seed.data_ptr() if seed is not None else 0)
    stream = ext._stream(0)
    mask = None
    if p > 0:
        mbuf = torch.full((B * L * S + 2 * GUARD,), 7, dtype=torch.uint8, device=DEV)
        assert lib.omnipq_attn_dropout_mask(N, H, L, S, p, seed_p, SALT, ctypes.c_void_p(mbuf.data_ptr() + GUARD), stream) == 0
        assert bool((mbuf[:GUARD] == 7).all()) and bool((mbuf[GUARD + B * L * S:] == 7).all())
        mask = mbuf[GUARD:GUARD + B * L * S].reshape(B, L, S).cpu()
        assert int(mask.max()) <= 1
    lse_buf, lse_p = f32_out(B, L)
    rc = lib.omnipq_attn_fwd(N, H, L, S, D, sl["q"].ptr(), sl["k"].ptr(), sl["v"].ptr(), sl["o"].ptr(), strides, lse_p, p,
                             seed_p, SALT, stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    got = dict(O=sl["o"].get(N, H), lse2=f32_get(lse_buf, B, L))
    assert untouched([sl[n] for n in ("q", "k", "v", "o")]), "forward wrote between the rows"
    assert bool(torch.isfinite(got["lse2"]).all()) and bool(torch.isfinite(got["O"].float()).all())
    delta_buf, delta_p = f32_out(B, L)
    rc = lib.omnipq_attn_bwd(N, H, L, S, D, sl["q"].ptr(), sl["k"].ptr(), sl["v"].ptr(), sl["o"].ptr(), sl["do"].ptr(),
                             strides, lse_p, delta_p, sl["dq"].ptr(), sl["dk"].ptr(), sl["dv"].ptr(), gstrides, p, seed_p,
                             SALT, stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    got.update(delta=f32_get(delta_buf, B, L), dQ=sl["dq"].get(N, H), dK=sl["dk"].get(N, H), dV=sl["dv"].get(N, H))
    assert untouched(list(sl.values())), "backward wrote between the rows"
    assert torch.equal(sl["o"].get(N, H).view(torch.int16), got["O"].view(torch.int16)), "backward changed O"
    assert torch.equal(f32_get(lse_buf, B, L), got["lse2"]), "backward changed lse2"
    return got, mask


def check(case):
    q, k, v, do = ar.case_inputs(case)
    got, mask = run_kernels(case, q, k, v, do)
    ref = ar.reference(q, k, v, do, mask, case["p"])
    bnd = ar.bounds(ref, case["dtype"], o_stored=got["O"])
    rat = ar.ratios(got, ref, bnd, o_stored=got["O"])
    lib = "f16" if case["dtype"] is torch.float16 else "bf16"
    print(f"\n  RATIO {lib} {case['id']}: {ar.fmt(rat)}")
    assert set(rat) == set(ar.OUTPUTS)
    assert not ar.outside(rat), (case["id"], ar.outside(rat))
    return got, mask, ref


@pytest.mark.parametrize("id", ar.CASE_IDS)
def test_every_element_is_inside_its_bound(id):
    case = ar.CASES[ar.CASE_IDS.index(id)]
    got, mask, ref = check(case)
    if case["p"] > 0:
        keep = float(mask.float().mean())
        n = mask.numel()
        assert abs(keep - (1 - case["p"])) < 5.0 * (case["p"] * (1 - case["p"]) / n) ** 0.5 + 1e-3, keep
    if id == "dropout-0.5-onekey":
        # one key: P = 1, so a query's output is exactly 0 (dropped) or v / (1 - p) rounded (kept), lse2 is the plain score
        q, k, v, do = ar.case_inputs(case)
        want = torch.where(mask.bool(), (2.0 * v.float()).to(v.dtype).expand(-1, case["L"], -1),
                           torch.zeros((), dtype=v.dtype))
        assert torch.equal(got["O"].float(), want.float())
        assert 0 < int(mask.sum()) < mask.numel()
        plain = ar.reference(q, k, v, do)               # without dropout
        assert float((got["lse2"].double() - plain["lse2"]).abs().max()) <= float(ar.bounds(plain, v.dtype)["lse2"].max())
        for n in ("dQ", "dK", "dV"):
            assert bool(torch.isfinite(got[n].float()).all()), n
    if id == "logits-equal":
        S = case["S"]
        s2 = (ref["c"] * ref["q"] @ ref["k"].transpose(1, 2))[:, :, 0] * ar.LOG2E
        assert float((got["lse2"].double() - (s2 + torch.log2(torch.tensor(float(S), dtype=torch.float64)))).abs().max()) \
            <= float(ar.bounds(ref, case["dtype"])["lse2"].max())


def test_same_seed_and_salt_same_mask_other_salt_another():
    """the mask entry point is a function of (seed, salt, shape, p) alone -- what lets the tests above hand the reference
    the mask the kernels drew"""
    lib, ext = lib_of(torch.bfloat16)
    N, H, L, S, p = 2, 2, 33, 130, 0.5
    seed = torch.tensor([SEED], dtype=torch.int64, device=DEV)
    masks = []
    for salt in (SALT, SALT, SALT + 1):
        m = torch.empty((N * H, L, S), dtype=torch.uint8, device=DEV)
        assert lib.omnipq_attn_dropout_mask(N, H, L, S, p, ctypes.c_void_p(seed.data_ptr()), salt,
                                            ctypes.c_void_p(m.data_ptr()), ext._stream(0)) == 0
        masks.append(m.cpu())
    assert torch.equal(masks[0], masks[1])
    assert 0.4 < float((masks[0] == masks[2]).float().mean()) < 0.6


def _packed_vs_plain(L, S, N, H, D, p, cross, dtype=torch.bfloat16):
    """fused_attention.PackedAttention (rows ordered (batch, token), q|k|v side by side) against fused_attention.attention
    on (tokens, batch, embed) copies of the same values: the same kernels on the same numbers in another layout."""
    import sa_fused
    from utils import fused_attention
    sa_fused.E16.select(dtype)
    E = H * D
    gen = torch.Generator().manual_seed(L + S)
    q = (1.5 * torch.randn((N, L, E), generator=gen)).to(dtype).to(DEV)
    Sk = S if cross else L
    k = (1.5 * torch.randn((N, Sk, E), generator=gen)).to(dtype).to(DEV)
    v = torch.randn((N, Sk, E), generator=gen).to(dtype).to(DEV)
    g = torch.randn((N, L, E), generator=gen).to(dtype).to(DEV)
    if cross:
        a = q.reshape(N * L, E).clone().requires_grad_(True)
        b = torch.cat([k, v], dim=2).reshape(N * Sk, 2 * E).contiguous().requires_grad_(True)
    else:
        a = torch.cat([q, k, v], dim=2).reshape(N * L, 3 * E).contiguous().requires_grad_(True)
        b = None
    assert fused_attention.packed_usable(a, b, H)
    tq, tk, tv = (t.transpose(0, 1).contiguous().requires_grad_(True) for t in (q, k, v))
    assert fused_attention.usable(tq, tk, tv, H)

    def state():
        fused_attention.STATE.set_state(DEV, 424242)
        fused_attention.STATE.advance(DEV)

    state()
    out_p = fused_attention.PackedAttention.apply(a, b, L, Sk, N, H, p)
    grads_p = torch.autograd.grad(out_p, [a] if b is None else [a, b], g.reshape(N * L, E))
    state()                                             # the same seed, and the salt counter back at zero
    out_t = fused_attention.attention(tq, tk, tv, H, p)
    dq, dk, dv = torch.autograd.grad(out_t, [tq, tk, tv], g.transpose(0, 1).contiguous())
    assert torch.equal(out_p.reshape(N, L, E), out_t.transpose(0, 1))
    dq, dk, dv = (t.transpose(0, 1) for t in (dq, dk, dv))
    if cross:
        assert torch.equal(grads_p[0].reshape(N, L, E), dq)
        assert torch.equal(grads_p[1].reshape(N, Sk, 2 * E), torch.cat([dk, dv], dim=2))
    else:
        assert torch.equal(grads_p[0].reshape(N, L, 3 * E), torch.cat([dq, dk, dv], dim=2))
    assert bool(torch.isfinite(out_p.float()).all()) and float(out_p.float().abs().max()) > 0
    if p > 0:                                           # ... and dropout was on: another salt, another output
        out2 = fused_attention.attention(tq, tk, tv, H, p)
        assert not torch.equal(out2, out_t)


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("cross", [False, True])
@pytest.mark.parametrize("L,S,N,H,D", [(70, 70, 2, 4, 36), (33, 130, 2, 4, 36)])
def test_packed_attention_is_bit_equal_to_the_strided_one(L, S, N, H, D, cross, p):
    _packed_vs_plain(L, S, N, H, D, p, cross)
