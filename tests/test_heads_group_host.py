"""CPU only: the host side of the grouped backward of the prediction heads.  pred_heads.heads_bwd_route decides from
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
    import pred_heads as pq
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


MOVED_SWITCHES = ("_JOINT_HEADS", "_HEAD_EVAL_CHAIN", "_FUSED_DECODE", "_PAIR_DECODE", "_PAIR_STACKS", "_XYZ_SINK", "_POS_ROWS16",
                  "_POS_KPAD", "_HEADS_BWD_GROUP", "_HEADS_GROUP_MAX")


def test_every_switch_of_the_heads_exists_in_one_module_only(built_lib):
    """(a copy in pq_transformer would be dead: `bench.py --set` and monkeypatch.setattr would set it and measure nothing)"""
    import pq_transformer
    import pred_heads
    for name in MOVED_SWITCHES:
        assert hasattr(pred_heads, name) and not hasattr(pq_transformer, name), name
    assert pq_transformer.PredictHead is pred_heads.PredictHead and pq_transformer.QuadPredictHead is pred_heads.QuadPredictHead
    assert pq_transformer.seat_head_parameters is pred_heads.seat_head_parameters
    assert pred_heads.PredictHead.__module__ == "pred_heads"


def _stage_route_restated(pair_decode, fused_decode, grouped, like_first, cuda, usable_a, usable_b, head_training, quad_training,
                          base_grad, has_sink):
    """The conditions as predict_pair, head_stack_pair and HeadsGroup.stage spelled them while they looked at tensors."""
    if grouped:                                            # predict_pair: a group was handed in -- HeadsGroup.stage
        refused = not (head_training and quad_training) or (base_grad and not has_sink)
        if not refused:
            refused = not (usable_a and usable_b)
        if not refused:
            refused = not like_first
        if not refused:
            return "group"
    if not (pair_decode and fused_decode and cuda):
        return "single"
    if usable_a and usable_b:                              # both stacks' rows come from the row kernels: the pair decode
        return "pair"
    return "stacks"


def test_stage_route_over_every_combination_of_its_inputs(built_lib, monkeypatch):
    import pred_heads
    n = 0
    for pair_decode, fused_decode in itertools.product((False, True), repeat=2):
        monkeypatch.setattr(pred_heads, "_PAIR_DECODE", pair_decode)
        monkeypatch.setattr(pred_heads, "_FUSED_DECODE", fused_decode)
        for facts in itertools.product((False, True), repeat=9):
            assert pred_heads.stage_route(*facts) == _stage_route_restated(pair_decode, fused_decode, *facts), \
                (pair_decode, fused_decode, facts)
            n += 1
    assert n == 2048
    # whether two usable stacks of one mode share their launches is the one reading of _PAIR_STACKS
    for on in (False, True):
        monkeypatch.setattr(pred_heads, "_PAIR_STACKS", on)
        for same_mode, ua, ub in itertools.product((False, True), repeat=3):
            assert pred_heads.stacks_paired(same_mode, ua, ub) is (on and same_mode and ua and ub)


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
        """the pair's forward outside autograd, as pred_heads runs a grouped stage -> (its tape, output gradients)"""
        ya, yb, tape = rows_mlp.tape_pair(xs[0], stacks[0], xs[1], stacks[1], True, padded=True)
        return tape, torch.ones_like(ya), torch.ones_like(yb)

    def programs(ctx, ga, gb, last):
        nig = (True, False, False) + (True,) * 12
        return list(rows_mlp.tape_programs(ctx, ga, gb, nig, nig, b_leads=not last))

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
