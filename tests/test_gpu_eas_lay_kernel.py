"""GPU: the EAS-Lay kernels one at a time -- the layer case of the start-sharing rollout kernel (csrc/rollout_multistart.hip,
k_rollout_ms_mfma<..., LayArgs>) through ops.rollout(eas_layer=), and eamrl_eas_layer_backward (csrc/eas_layer.hip) through
ops.ReevalPlan.backward_layer.

Forward: per-step log-probs of the kernel's own actions (greedy, and the same tours fed back in evaluate mode) against the
float64 restatement tests/eas_layer_ref.py on the rollout's own cache tensors, 1e-5 (the header's contract for log-probs).  The
captured heads are the PRE-layer glimpse outputs: against the plain kernel's capture on the same tours they agree to 1e-6 of the
largest entry, not bit for bit -- the layer instantiations use the fixed node chunks of the PolyNet case.  With
W2 = b2 = 0 the log-probs are eamrl_reeval_forward's of the same actions (1e-5).  The forced row changes no other row, bit for bit.

Backward: all four gradients in every case of tests/eas_layer_cases.py against float64, with reeval_cases' rule: MARGIN = 4 times
the float32 restatement's own error, by norm.  Every figure is printed before it is asserted.

Measured on the MI355X, kernel error / error of the restatement's float32 run (norm of the difference), the largest over the 7
cases and the case it occurs in:
  dW1    1.93  lay_M20_S5_B100_nchunk1
  db1    1.98  lay_M20_S5_B100_nchunk1
  dW2    2.31  lay_M20_S5_B100_nchunk1
  db2    2.32  lay_M20_S5_B100_nchunk1
All inside MARGIN = 4; the cases with a recovered normaliser (lse == NULL) stay below 1.9.  Forward: log-probs 4.3e-7 .. 6.8e-7 from
float64 (bound 1e-5), captured heads 3.0e-7 .. 3.6e-7 from the plain kernel's (|h| up to 1.5), zero residual 1.4e-6 .. 1.9e-6 from
eamrl_reeval_forward.
"""
import functools

import pytest
import torch

import eas_layer_cases as ec
import eas_layer_ref as er
import reeval_ref as rr

pytestmark = pytest.mark.gpu

DEV = "cuda"
E = er.E


def dev(x):
    return None if x is None else x.to(DEV).contiguous()


# ---- forward: the layer rollout on a policy's own cache -------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def searcher(env_name, num_loc, B, n_aug):
    """An EASLay search state on golden-weight policy: (eas, state, layer weights of the reference's shapes with non-zero W2)."""
    import eam_rl4co_amd as ea
    from test_gpu_parity import make_policy

    torch.manual_seed(11)
    env = ea.get_env(env_name, generator_params=dict(num_loc=num_loc))
    td = env.reset(batch_size=[B]).to(DEV)
    eas = ea.EASLay(env, make_policy("am_" + env_name), augment_size=n_aug, augment_dihedral=n_aug == 8)
    s = eas.begin(td, seed=5)
    g = torch.Generator().manual_seed(77)
    lay = dict(W1=torch.randn(s.Ba, E, E, generator=g) * 0.1, b1=torch.randn(s.Ba, E, generator=g) * 0.3,
               W2=torch.randn(s.Ba, E, E, generator=g) * 0.05, b2=torch.randn(s.Ba, E, generator=g) * 0.1)
    return eas, s, lay


def operands_of(lay, zero_residual=False, forced=None):
    from eam_rl4co_amd import ops

    z = torch.zeros_like
    return ops.eas_layer_operands(dev(lay["W1"]), dev(lay["b1"]), dev(z(lay["W2"]) if zero_residual else lay["W2"]),
                                  dev(z(lay["b2"]) if zero_residual else lay["b2"]), forced=forced)


def roll(eas, s, mode, start, layer=None, given=None, seed=None):
    """One rollout of len(start) / Ba rows per instance behind the given start column.
    -> actions [R, T] (start column included), logp [R, T], heads [R, >= T - 1, E], status"""
    from eam_rl4co_amd import ops
    from eam_rl4co_amd.policy import _env_step_, _max_decode_steps, state_from_td

    pol = eas.policy
    st = state_from_td(pol.env_name, s.td, start.numel() // s.Ba)
    _env_step_(st, start)
    t_max = int(max(1, _max_decode_steps(pol.env_name, s.M, 1)))
    acts, lps, info = ops.rollout(st, s.cache, mode, given=given, clip=pol.tanh_clipping, temp=pol.temperature, t_max=t_max, seed=seed,
                                  want_heads=True, eas_layer=layer)
    T, status = info.tolist()
    actions = torch.cat((start[:, None], acts[:, :T]), 1).contiguous()
    logp = torch.cat((torch.zeros_like(lps[:, :1]), lps[:, :T]), 1).contiguous()
    return actions, logp, st.heads, status


def starts(eas, s, extra=None):
    st = eas.env.select_start_nodes(s.td, num_starts=s.S).to(torch.int64)
    return (st if extra is None else torch.cat((st, extra))).contiguous()


def float64_logp(eas, s, actions, S1, lay):
    """The restatement's log-probs [R, T] of `actions` on the rollout's own cache, in float64."""
    plan = eas._plan(s, actions, S1)
    c = s.cache
    R, T = actions.shape
    bits = plan.maskbits.cpu().numpy().view("uint32")
    mask = torch.from_numpy(((bits[..., None] >> torch.arange(32).numpy().astype("uint32")) & 1).astype(bool)).reshape(R, T, 128)[..., :s.M]
    cpu = lambda x: None if x is None else x.detach().cpu()
    op = dict(K=cpu(c.view("K")), V=cpu(c.view("V")), Lp=cpu(c.view("Lp")), Pa=cpu(c.view("Pa")),
              Pb=cpu(c.view("Pb")) if plan.has_pb else None, gctx=cpu(plan.gctx), Cvec=cpu(plan.cvec) if plan.NC else None,
              sc=cpu(plan.sc) if plan.NC else None, idxA=cpu(plan.idxA), idxB=cpu(plan.idxB) if plan.has_pb else None, mask=mask,
              actions=cpu(actions), S=S1, tstart=plan.tstart, clip=plan.clip, temp=plan.temp, rem=None, dyn=None, heads=None)
    op64 = rr.cast(op, torch.float64)
    heads = rr.reeval(op64)["heads"]
    return er.forward(op64, er.cast(lay, torch.float64), heads)["logp"], heads


SHAPES = [("tsp", 20, 2, 8), ("cvrp", 20, 2, 8), ("tsp", 50, 1, 2), ("cvrp", 100, 1, 2)]       # 2, 2, 4 and 7 key tiles


@pytest.mark.parametrize("env_name,num_loc,B,n_aug", SHAPES)
def test_layer_rollout_log_probs_against_float64(env_name, num_loc, B, n_aug):
    from eam_rl4co_amd import ops

    eas, s, lay = searcher(env_name, num_loc, B, n_aug)
    layer = operands_of(lay)
    start = starts(eas, s)
    acts, lp, heads, status = roll(eas, s, "greedy", start, layer)
    ops.raise_on_status(status)
    ref, heads64 = float64_logp(eas, s, acts, s.S, lay)
    err = float((lp.cpu().double() - ref).abs().max())
    T = acts.shape[1]
    cap = heads[:, :T - 1].cpu().double()
    live = cap.abs().sum(-1) > 0                           # (a row that is done has zeros in the capture)
    assert bool(live.all()) or env_name != "tsp"
    herr = float((cap - heads64[:, 1:])[live].abs().max())
    acts_e, lp_e, heads_e, status_e = roll(eas, s, "evaluate", start, layer, given=acts[:, 1:].contiguous())
    same = torch.equal(acts_e, acts) and torch.equal(lp_e.view(torch.int32), lp.view(torch.int32))
    print(f"EASLAYF {env_name}{num_loc}: greedy log-probs against float64 {err:.3e} (bound 1e-5); captured heads against float64 {herr:.3e}; "
          f"evaluate of the same tours bit-identical {same}")
    assert status_e == 0 and err <= 1e-5 and same
    assert herr <= 1e-5        # (the live steps' pre-layer heads; a done row's are zero on both sides)


@pytest.mark.parametrize("env_name,num_loc,B,n_aug", SHAPES)
def test_captured_heads_are_the_pre_layer_heads_of_the_plain_kernel(env_name, num_loc, B, n_aug):
    eas, s, lay = searcher(env_name, num_loc, B, n_aug)
    start = starts(eas, s)
    acts, _, _, _ = roll(eas, s, "greedy", start, operands_of(lay))
    given = acts[:, 1:].contiguous()
    _, _, h_lay, st1 = roll(eas, s, "evaluate", start, operands_of(lay), given=given)
    _, _, h_plain, st0 = roll(eas, s, "evaluate", start, None, given=given)
    assert st0 == 0 and st1 == 0 and h_lay.shape == h_plain.shape
    top = float(h_plain.abs().max())
    err = float((h_lay - h_plain).abs().max())
    print(f"EASLAYH {env_name}{num_loc}: captured heads with / without the layer: max diff {err:.3e}, max |h| {top:.3e}, "
          f"bit-identical {torch.equal(h_lay, h_plain)}")
    assert top > 0 and err <= 1e-6 * top


@pytest.mark.parametrize("env_name", ["tsp", "cvrp"])
def test_zero_residual_is_the_plain_decode_step(env_name):
    eas, s, lay = searcher(env_name, 20, 2, 8)
    acts, lp, _, status = roll(eas, s, "sampling", starts(eas, s), operands_of(lay, zero_residual=True), seed=123)
    plan = eas._plan(s, acts, s.S)
    ref = plan.forward()
    err = float((lp - ref).abs().max())
    print(f"EASLAYZ {env_name}: W2 = b2 = 0 against eamrl_reeval_forward {err:.3e} (bound 1e-5)")
    assert status == 0 and err <= 1e-5


@pytest.mark.parametrize("env_name", ["tsp", "cvrp"])
def test_forced_row_follows_its_tour_and_leaves_the_others_alone(env_name):
    from eam_rl4co_amd import ops

    eas, s, lay = searcher(env_name, 20, 2, 8)
    tours, _, _, _ = roll(eas, s, "greedy", starts(eas, s), operands_of(lay))
    tour = tours[:s.Ba]                                     # the first start's greedy tour of every augmented instance
    start = starts(eas, s, extra=tour[:, 0])
    forced = tour[:, 1:].contiguous()
    a0, l0, _, st0 = roll(eas, s, "sampling", start, operands_of(lay), seed=99)
    a1, l1, _, st1 = roll(eas, s, "sampling", start, operands_of(lay, forced=forced), seed=99)
    assert st0 == 0 and st1 == 0 and a0.shape == a1.shape
    n = s.S * s.Ba
    assert torch.equal(a0[:n], a1[:n]) and torch.equal(l0[:n].view(torch.int32), l1[:n].view(torch.int32))
    T = a1.shape[1]
    want = torch.zeros(s.Ba, T, dtype=torch.int64, device=DEV)
    w = min(T, tour.shape[1])
    want[:, :w] = tour[:, :w]
    assert torch.equal(a1[n:], want) and not torch.equal(a0[n:], a1[n:])
    ref, _ = float64_logp(eas, s, a1, s.S + 1, lay)
    err = float((l1.cpu().double() - ref).abs().max())
    print(f"EASLAYR {env_name}: forced row = its tour, the other {n} rows bit-identical; log-probs against float64 {err:.3e}")
    assert err <= 1e-5
    # a short forced tour is padded with the depot / node 0: t_forced = 3
    a2, _, _, st2 = roll(eas, s, "sampling", start, operands_of(lay, forced=forced[:, :3].contiguous()), seed=99)
    assert torch.equal(a2[n:, :4], tour[:, :4]) and (a2[n:, 4:] == 0).all()
    assert (st2 & ops.ST_INFEASIBLE) != 0 if env_name == "tsp" else True       # TSP: node 0 again and again is infeasible
    bad = forced.clone()
    bad[:, 1] = bad[:, 0]                                   # the same customer twice
    _, _, _, st3 = roll(eas, s, "sampling", start, operands_of(lay, forced=bad), seed=99)
    with pytest.raises(AssertionError, match="infeasible"):
        ops.raise_on_status(st3)


def test_layer_rollout_refuses_what_is_not_built():
    from eam_rl4co_amd import ops

    eas, s, lay = searcher("tsp", 20, 2, 8)
    layer = operands_of(lay)
    with pytest.raises(NotImplementedError, match="top-k / top-p"):
        roll_kw = dict(clip=10.0, temp=1.0, t_max=20, eas_layer=layer, top_k=3)
        from eam_rl4co_amd.policy import state_from_td
        ops.rollout(state_from_td("tsp", s.td, s.S), s.cache, "greedy", **roll_kw)
    with pytest.raises(NotImplementedError, match="rows per instance"):
        roll(eas, s, "greedy", starts(eas, s)[:s.Ba], layer)             # one row per instance
    with pytest.raises(ValueError, match="one layer per instance"):
        roll(eas, s, "greedy", starts(eas, s), {k: v[:1] for k, v in layer.items()})


# ---- backward: eamrl_eas_layer_backward on the cases ----------------------------------------------------------------------------------
def make_plan(name, zero_w2=False, heads=True):
    from eam_rl4co_amd import ops

    c = ec.CASES[name]
    op, glogp, lay, hd, r64, _ = ec.reference(name)
    names = ["K", "V", "Lp", "Pa"] + (["Pb"] if c["pb"] else [])
    buf = dev(torch.cat([op[k] for k in names], dim=-1))
    t0 = c["tstart"]
    plan = ops.ReevalPlan(buf, c["pb"], dev(op["gctx"]), dev(op["Cvec"]), dev(op["idxA"]), dev(op["idxB"]), dev(op["sc"]),
                          dev(rr.pack_mask_bits(op["mask"].numpy())), dev(op["actions"]), c["S"], t0, c["clip"], c["temp"],
                          rollout_logp=dev(r64["logp"].float()), rollout_heads=dev(hd[:, t0:]) if heads else None, E=E)
    if c["lse"]:
        plan.lse = dev(r64["lse"].float())
    if c["nchunk"] is not None:
        plan.nchunk = c["nchunk"]
    W2 = torch.zeros_like(lay["W2"]) if zero_w2 else lay["W2"]
    layer = ops.eas_layer_operands(dev(lay["W1"]), dev(lay["b1"]), dev(W2), dev(lay["b2"]))
    return plan, dev(glogp), layer


def unpacked(got):
    from eam_rl4co_amd import ops

    return {"dW1": ops.unpack_eas_layer(got["W1"]).cpu(), "db1": got["b1"].cpu(), "dW2": ops.unpack_eas_layer(got["W2"]).cpu(),
            "db2": got["b2"].cpu()}


def check(name, got, tag):
    _, _, _, _, r64, r32 = ec.reference(name)
    bad = []
    for g in er.GRADS:
        fig = float((got[g].double() - r64[g]).norm())
        f32 = float((r32[g].double() - r64[g]).norm())
        bd = ec.bound(name, g, r64, r32)
        print(f"{tag} {name} {g} kernel {fig:.3e} float32-restatement {f32:.3e} ratio {fig / f32:.2f} bound {bd:.3e} ref {float(r64[g].norm()):.3e}")
        assert torch.isfinite(got[g]).all()
        if not fig <= bd:
            bad.append((g, fig, bd))
    return bad


@pytest.mark.parametrize("name", ec.NAMES)
def test_backward_layer_matches_the_float64_restatement(name):
    plan, g, layer = make_plan(name)
    assert (plan.lse is None) == (not ec.CASES[name]["lse"])
    got = unpacked(plan.backward_layer(g, layer))
    assert check(name, got, "EASLAYB") == []


@pytest.mark.parametrize("name", ["lay_M20_S2_B3", "lay_M20_S5_B100_nchunk1"])
def test_backward_layer_accumulates_into_out(name):
    plan, g, layer = make_plan(name)
    c = ec.CASES[name]
    out = {n: torch.zeros(c["B"], E * (E if n[0] == "W" else 1), device=DEV) for n in er.PARAMS}
    assert plan.backward_layer(g, layer, out=out) is out
    plan.backward_layer(g, layer, out=out)
    assert check(name, {k: v / 2 for k, v in unpacked(out).items()}, "EASLAYA") == []       # (halving is exact)


@pytest.mark.parametrize("name", ["lay_M33_S16_B3", "lay_M112_S4_B3_forced_logp"])
def test_zero_w2_gives_exactly_zero_dw1_and_db1(name):
    plan, g, layer = make_plan(name, zero_w2=True)
    got = plan.backward_layer(g, layer)
    assert (got["W1"] == 0).all() and (got["b1"] == 0).all()
    assert float(got["W2"].abs().max()) > 0 and float(got["b2"].abs().max()) > 0


def test_steps_that_take_no_gradient_contribute_exact_zeros():
    """glogp non-zero only at steps before tstart and at the steps with a single feasible node: all four gradients stay zero."""
    import reeval_cases as rc

    name = "lay_M112_S4_B3_forced"
    plan, g, layer = make_plan(name)
    T = ec.CASES[name]["T"]
    t = torch.arange(T)
    dead = (t < ec.CASES[name]["tstart"]) | (t % rc.FORCED_EVERY[0] == rc.FORCED_EVERY[1])
    got = plan.backward_layer(g * dev(dead.float())[None, :], layer)
    assert all((got[n] == 0).all() for n in er.PARAMS)


def test_refusals_launch_nothing():
    from test_gpu_eas_kernel import make_plan as make_lp_plan

    name = "lay_M20_S2_B3"
    c = ec.CASES[name]
    zeros = lambda B: {n: torch.zeros(B, E * (E if n[0] == "W" else 1), device=DEV) for n in er.PARAMS}
    plan, g, layer = make_plan(name, heads=False)
    out = zeros(c["B"])
    with pytest.raises(RuntimeError, match=r"eamrl_eas_layer_backward.*heads != nullptr"):
        plan.backward_layer(g, layer, out=out)
    plan, g, layer = make_plan(name)
    plan.dyn, plan.rem = torch.zeros(3, E, device=DEV), torch.zeros(plan.R, plan.T, 128, device=DEV)
    with pytest.raises(RuntimeError, match=r"eamrl_eas_layer_backward.*dyn == nullptr"):
        plan.backward_layer(g, layer, out=out)
    big, gb = make_lp_plan("edge_M113")
    out_b = zeros(big.B)
    lay_b = {n: torch.zeros_like(v) for n, v in out_b.items()}
    with pytest.raises(RuntimeError, match=r"eamrl_eas_layer_backward.*M <= 112"):
        big.backward_layer(gb, lay_b, out=out_b)
    torch.cuda.synchronize()
    assert all((v == 0).all() for v in out.values()) and all((v == 0).all() for v in out_b.values())
