"""CPU: the cases of tests/encoder16_cases.py can tell a wrong 16-bit fused encoder from a right one.

The exact cases carry a certificate that every GEMM is exact in fp32 in any order (so bit equality with the float64
emulation is a fair demand on the kernel) and an adversary that makes the padded-key mask matter.  Every one-line variant of
the contract in precision_emulation.MUTANTS is rejected by a named case with the very comparison that
test_gpu_encoder16_contract.py applies to the kernel: bit inequality on an exact case, or a per-row error above the bound in
at least a tenth of the rows of a policy-scale case."""
import ast
import inspect

import numpy as np
import pytest

import encoder16_cases as cases
import precision_emulation as emu
from _util import golden_weights

EXACT = {cases.exact_id(c): c for c in cases.EXACT_CASES}
POLICY = {cases.policy_id(c): c for c in cases.POLICY_CASES}


@pytest.mark.parametrize("case", cases.EXACT_CASES, ids=cases.exact_id)
def test_exact_case_certificate_adversary_and_flag(case):
    moved = set()
    for kind in cases.KINDS:
        out, tr = cases.exact_reference(case, kind)
        assert cases.certificate(tr) is None, (kind, cases.certificate(tr))
        assert set(tr.gemm) >= {"qkv", "scores", "value product", "out_proj", "ffn1", "ffn2"}
        if case.nproj:
            assert set(tr.gemm) >= set(cases.CACHE_SLOTS[case.nproj]) | ({"gctx"} if case.gctx else set())
        for name, v in out.items():
            assert np.array_equal(v, v.astype(np.float32)), f"{kind} {name}: not fp32 numbers"
        if emu.padded_rows(case.M) > case.M:
            # without this a wrong mask goes unseen: an unmasked key that does not hold the maximum has weight exactly 0
            assert tr.adversary >= 0.25, f"{kind}: padded keys would win only {tr.adversary:.0%} of (query, head) pairs"
        moved |= tr.rounded
        if case.rounding_free:
            assert tr.max_tie <= 2
            plain, _ = cases.exact_reference(case, None)
            assert all(np.array_equal(out[n], plain[n]) for n in out), f"{kind}: differs from the unrounded run"
    assert case.rounding_free == (not moved), f"rounding points that move a value: {sorted(moved)}"


def test_exact_cases_cover_the_variants_and_their_edges():
    Ms = {c.M for c in cases.EXACT_CASES}
    assert Ms >= {1, 15, 16, 17, 31, 32} | {33, 47, 48, 49, 64} | {65, 80, 81, 96, 97, 111, 112}
    free = {emu.padded_rows(c.M) for c in cases.EXACT_CASES if c.rounding_free}
    assert free == {32, 64, 112}, "a rounding-free case for every kernel variant"
    assert {c.nproj for c in cases.EXACT_CASES} == {0, 4, 5} and {c.B for c in cases.EXACT_CASES} == {1, 3}
    assert {bool(c.pad) for c in cases.EXACT_CASES if c.nproj} == {False, True}
    assert all(c.M & (c.M - 1) == 0 for c in cases.EXACT_CASES if c.gctx) and any(c.gctx for c in cases.EXACT_CASES)
    assert any(cases.exact_reference(c, "fp16")[1].max_tie >= 3 for c in cases.EXACT_CASES), \
        "no case divides by a tie of 3: the fp32 division is not exercised"


def test_exact_case_seeds_are_literals():
    """The table is written out, not searched at import: a seed that stops passing the certificate fails the test above."""
    tree = ast.parse(inspect.getsource(cases))
    table = [n for n in ast.walk(tree) if isinstance(n, ast.Assign) and getattr(n.targets[0], "id", "") == "EXACT_CASES"]
    assert len(table) == 1 and len(table[0].value.elts) == len(cases.EXACT_CASES)
    for call in table[0].value.elts:
        assert isinstance(call, ast.Call) and call.func.id == "ExactCase" and not call.keywords
        assert all(isinstance(a, ast.Constant) for a in call.args)


# mutant -> the named cases that must reject it: ("exact", case id, kind) or ("policy", case id, kind)
REJECTED_BY = {
    "unmasked": [("exact", "M17-B3-nproj5-pad24", "bf16"), ("exact", "M65-B3-nproj4-pad0", "fp16")],
    "mask_m1": [("exact", "M17-B3-nproj5-pad24", "bf16"), ("exact", "M112-B3-nproj5-pad0", "fp16")],
    "mask_p1": [("exact", "M15-B3-nproj4-pad24", "bf16"), ("exact", "M111-B3-nproj4-pad24", "fp16")],
    "pad_tile": [("exact", "M48-B3-nproj5-pad0", "bf16"), ("exact", "M96-B3-nproj4-pad0", "fp16"),
                 ("exact", "M16-B3-nproj5-pad0-gctx", "bf16")],
    "heads_swapped": [("exact", "M33-B3-nproj5-pad24", "bf16"), ("exact", "M33-B3-nproj4-pad0-light", "fp16")],
    "tiles_swapped": [("exact", "M33-B3-nproj5-pad24", "bf16"), ("exact", "M112-B3-nproj5-pad0-light", "fp16")],
    "w1_chunks": [("exact", "M33-B3-nproj5-pad24", "bf16"), ("exact", "M1-B3-nproj4-pad0-light", "fp16")],
    "lp_unrounded_l": [("exact", "M15-B3-nproj4-pad24", "bf16"), ("exact", "M80-B3-nproj5-pad0", "fp16")],
    "lp_from_k": [("exact", "M15-B3-nproj4-pad24", "bf16"), ("exact", "M17-B3-nproj5-pad0-light", "fp16")],
    "w_unrounded": [("policy", "attention-batch-M17", "bf16"), ("policy", "attention-batch-M112", "bf16")],
    "z_unrounded": [("policy", "attention-batch-M17", "bf16"), ("policy", "attention-batch-M112", "bf16")],
    "hidden_unrounded": [("exact", "M15-B3-nproj4-pad24", "bf16"), ("policy", "ffn-batch-M17", "bf16")],
    "input_unrounded": [("exact", "M15-B3-nproj4-pad24", "fp16"), ("policy", "attention-batch-M17", "bf16")],
    "bias_rounded": [("policy", "cache-batch-M33", "bf16"), ("policy", "attention-batch-M97", "bf16")],
    "residual_rounded": [("exact", "M15-B3-nproj4-pad24", "bf16"), ("policy", "cache-batch-M17", "bf16")],
    "o_unrounded": [("exact", "M15-B3-nproj4-pad24", "bf16"), ("policy", "attention-batch-M17", "bf16")],
}


def _rejects(how, cid, kind, mutant):
    if how == "exact":
        ref, _ = cases.exact_reference(EXACT[cid], kind)
        mut, _ = cases.exact_reference(EXACT[cid], kind, mutant)
        return any(not np.array_equal(ref[n], mut[n]) for n in ref)
    case = POLICY[cid]
    ratios = cases.policy_ratios(case, kind, cases.policy_reference(case, kind, mutant))
    factor = cases.policy_factor(case.stage, case.norm, kind)
    return any((r > factor.get(n, cases.POLICY_FACTOR)).mean() >= 0.1 for n, r in ratios.items())


@pytest.mark.parametrize("mutant", emu.MUTANTS)
def test_every_mutant_of_the_contract_is_rejected(mutant):
    assert set(REJECTED_BY) == set(emu.MUTANTS)
    for how, cid, kind in REJECTED_BY[mutant]:
        assert _rejects(how, cid, kind, mutant), f"{mutant} passes {how} case {cid} ({kind})"
        assert not _rejects(how, cid, kind, None)


def test_the_contract_itself_passes_every_comparison():
    """The yardstick run (fp32 accumulation, same rounding points) stays inside the bound it defines, by construction, and
    the division mirror moves nothing on policy-scale data: the comparisons reject mutants, not noise."""
    for case in cases.POLICY_CASES[::23]:
        for kind in cases.KINDS:
            h, layers, cache, eps = cases.policy_inputs(case)
            a32 = emu.run_contract(layers, h, emu.ROUNDING[kind], case.norm, eps, cache, acc=np.float32)
            assert all(r.max() <= 1.0 for r in cases.policy_ratios(case, kind, a32).values())
            d32 = emu.run_contract(layers, h, emu.ROUNDING[kind], case.norm, eps, cache, div32=True)
            assert all(r.max() <= cases.POLICY_FACTOR for r in cases.policy_ratios(case, kind, d32).values())


def test_d_expf_port():
    x = np.float32([0.0, -87.0, -87.5, -128.0, -np.inf])
    y = emu.d_expf(x)
    assert y[0] == 1.0 and y[1] > 0 and (y[2:] == 0).all()
    x = -np.abs(np.random.default_rng(0).standard_normal(4096) * 20).astype(np.float32)
    x = x[x >= -87]
    assert np.abs(emu.d_expf(x) / np.exp(x.astype(np.float64)) - 1).max() < 2e-7


@pytest.mark.parametrize("cfg,env_name", [("am_tsp", "tsp"), ("pomo_cvrp", "cvrp")])
def test_stagewise_form_is_the_state_dict_form(cfg, env_name):
    """run_contract on unpacked layers = encode + precompute on the policy's state dict (the form that
    test_host_precision.py holds to the oracle), with and without rounding."""
    sd = golden_weights(cfg)
    layers, li = [], 0
    while f"encoder.net.layers.{li}.0.module.Wqkv.weight" in sd:
        p = f"encoder.net.layers.{li}."
        Ly = {}
        for name, bias, key in (("Wqkv", "bqkv", "0.module.Wqkv"), ("Wo", "bo", "0.module.out_proj"),
                                ("W1", "b1", "2.module.lins.0"), ("W2", "b2", "2.module.lins.1")):
            Ly[name], Ly[bias] = sd[p + key + ".weight"], sd[p + key + ".bias"]
        for n, q in (("n1", "1"), ("n2", "3")):
            Ly[n + "_gamma"], Ly[n + "_beta"] = sd[p + q + ".normalizer.weight"], sd[p + q + ".normalizer.bias"]
            if p + q + ".normalizer.running_mean" in sd:
                Ly[n + "_mean"], Ly[n + "_var"] = sd[p + q + ".normalizer.running_mean"], sd[p + q + ".normalizer.running_var"]
        layers.append(Ly)
        li += 1
    norm = "batch" if "n1_mean" in layers[0] else "instance"
    E = cases.E
    Wctx = sd["decoder.context_embedding.project_context.weight"]
    nproj = 5 if env_name == "tsp" else 4
    Wc = np.concatenate([sd["decoder.project_node_embeddings.weight"]] + [Wctx[:, i * E:(i + 1) * E] for i in range(nproj - 3)])
    cache = dict(Wc=Wc, WoutT=sd["decoder.pointer.project_out.weight"].T, nproj=nproj,
                 Wg=sd["decoder.project_fixed_context.weight"])
    h = np.random.default_rng(3).standard_normal((2, 21, E)).astype(np.float32)
    for rnd in (None, emu.round_bf16, emu.round_fp16):
        new = emu.run_contract(layers, h, rnd, norm, 1e-5, cache)
        old_h = emu.encode(sd, h, rnd)
        old = emu.precompute(sd, env_name, old_h, rnd)
        old["h"] = old_h
        for name, v in new.items():
            assert emu.rel_err(v, old[name]) <= 1e-12, name
