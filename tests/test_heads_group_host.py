"""CPU only: the host side of the grouped backward of the prediction heads.  pq_transformer.heads_bwd_route decides from
flags alone; rows_mlp._lockstep runs n backward programs round by round -- on the recorder of
tests/golden/make_golden_rows_calls.py (nothing is launched) the calls of three pairs run as ONE lockstep are the calls of the
three pairs run one after the other, interleaved round by round, with every program but the last one leading."""
import importlib.util
import itertools
import os

from conftest import GOLDEN


def _generator():
    spec = importlib.util.spec_from_file_location("make_golden_rows_calls", os.path.join(GOLDEN, "make_golden_rows_calls.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_route_is_a_function_of_its_flags(built_lib, monkeypatch):
    import pq_transformer as pq
    assert pq._HEADS_BWD_GROUP is True                                       # ships on
    on = dict(stages=7, pair_stacks=True, pair_decode=True, fused_decode=True, cuda=True, training=True, grad=True, world=1,
              force_collectives=False)
    assert pq.heads_bwd_route(**on) == "group"
    for name in ("pair_stacks", "pair_decode", "fused_decode", "cuda", "training", "grad"):
        assert pq.heads_bwd_route(**dict(on, **{name: False})) == "stage", name
    assert pq.heads_bwd_route(**dict(on, world=2)) == "stage"               # the statistics exchange is made per pair
    assert pq.heads_bwd_route(**dict(on, force_collectives=True)) == "stage"
    assert pq.heads_bwd_route(**dict(on, stages=1)) == "group"
    assert pq.heads_bwd_route(**dict(on, stages=8)) == "stage"              # 16 stacks: more than a group holds
    assert pq.heads_bwd_route(**dict(on, stages=0)) == "stage"
    monkeypatch.setattr(pq, "_HEADS_BWD_GROUP", False)
    assert pq.heads_bwd_route(**on) == "stage"
    assert 2 * pq._HEADS_GROUP_MAX == 14                                     # csrc/common.h: kHeldMax


def _rounds(events):
    """a program pair's recorded events -> its rounds: a program's round ends with the call that follows its hold"""
    out, cur, held = [], [], False
    for ev in events:
        cur.append(ev)
        if isinstance(ev, str):
            assert ev.startswith("hold:") and not held
            held = True
        elif held:
            out.append(cur)
            cur, held = [], False
    assert not held
    return out, cur


def test_lockstep_of_n_programs_interleaves_the_pairs(built_lib):
    import torch
    import dropout_state
    import rows_mlp
    import sa_fused
    import pq_transformer as pq
    gen = _generator()
    rec = gen.Recorder()
    patches = [(rows_mlp, "_call", rec.call), (sa_fused, "_call", rec.call), (rows_mlp, "_hold", rec.hold),
               (rows_mlp, "zeros_f32", lambda n, device: torch.zeros(n)),
               (sa_fused, "zeros_f32", lambda n, device: torch.zeros(n)),
               (sa_fused, "zeros_f64", lambda rows, cols, device: torch.zeros(rows, cols, dtype=torch.float64))]
    torch.manual_seed(0)
    dropout_state.STATE.reset()
    pairs = []
    for _ in range(3):
        stacks = [gen._build(torch, rows_mlp, sa_fused, st, 0.0) for st in (gen.PAIR_A, gen.PAIR_B)]
        xs = [torch.empty(st[2], st[0], dtype=torch.bfloat16).requires_grad_(True) for st in (gen.PAIR_A, gen.PAIR_B)]
        pairs.append((stacks, xs))

    def forward(stacks, xs):
        """the pair's forward outside autograd, as pq_transformer.HeadsGroup runs it -> (its context, output gradients)"""
        ctx = pq._Taped()
        spec_a, params_a = rows_mlp._spec_of(xs[0], stacks[0], True, True)
        spec_b, params_b = rows_mlp._spec_of(xs[1], stacks[1], True, True)
        with torch.no_grad():
            ya, yb = rows_mlp.RowsMLPPair.forward(ctx, xs[0], spec_a, xs[1], spec_b, True, len(params_a), *params_a, *params_b)
        return ctx, torch.ones_like(ya), torch.ones_like(yb)

    def programs(ctx, ga, gb, last):
        nig = (True, False, False) + (True,) * 12
        return [rows_mlp._backward_program(ctx.a, True, ga, nig), rows_mlp._backward_program(ctx.b, not last, gb, nig)]

    with gen._patched(patches):
        # each pair on its own: a lockstep of two
        single = []
        for stacks, xs in pairs:
            ctx, ga, gb = forward(stacks, xs)
            del rec.events[:]
            outs = rows_mlp._lockstep(*programs(ctx, ga, gb, True))
            assert len(outs) == 2 and all(o[0] is not None for o in outs)
            single.append(list(rec.events))
        # the three pairs as one lockstep of six
        ctxs = [forward(stacks, xs) for stacks, xs in pairs]
        del rec.events[:]
        progs = list(itertools.chain.from_iterable(programs(*c, last=(i == 2)) for i, c in enumerate(ctxs)))
        outs = rows_mlp._lockstep(*progs)
        grouped = list(rec.events)
    assert len(outs) == 6 and all(o[0] is not None and len(o) == 3 + 12 for o in outs)
    assert sa_fused._lib.omnipq_pair_held() == 0                 # nothing held at the end
    split = [_rounds(ev) for ev in single]
    n_rounds = len(split[0][0])
    assert n_rounds == 2 * 5 and all(len(r) == n_rounds and tail == [] for r, tail in split)      # five launches per stack
    want = []
    for r in range(0, n_rounds, 2):                              # a pair's rounds alternate: its leader's, its follower's
        for p, (rounds, _) in enumerate(split):
            for half in (0, 1):
                last = p == 2 and half == 1
                want += ["hold:%d" % (not last) if isinstance(ev, str) else ev for ev in rounds[r + half]]
    assert len(grouped) == len(want)
    assert [i for i, (g, w) in enumerate(zip(grouped, want)) if g != w] == []
    # every hold is matched: a call follows it at once, and only the last program of a round does not lead
    holds = [i for i, ev in enumerate(grouped) if isinstance(ev, str)]
    assert len(holds) == 6 * 5 and all(not isinstance(grouped[i + 1], str) for i in holds)
    assert [grouped[i] for i in holds] == (["hold:1"] * 5 + ["hold:0"]) * 5
