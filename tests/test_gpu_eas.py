"""GPU: the EAS-Emb search (eam_rl4co_amd/search.py) piece by piece -- one iteration's logit-key gradient on the fast path
(eamrl_reeval_backward_lp) against autograd through the PyTorch re-evaluation (train._logp_rows) of the same tours with the loss
as the reference writes it (zoo/eas/search.py:223-241), the general path (train._NativeReeval) against the fast one, and whole
searches: valid incumbents whose reward is max_reward bit for bit, never worse than iteration 0's, on an untouched policy.
Tolerance of the gradients: the native-versus-autograd contract of tests/test_gpu_train.py, atol = 1e-4 max|ref|.

Measured on the MI355X (TSP-20 / CVRP-20, B = 2, dihedral-8; max|ref| 2.0e-2 .. 5.1e-2): fast path against autograd 1.1e-8 .. 2.4e-8,
general path against fast path 2.8e-9 .. 1.9e-8 -- about 5e-7 of the largest entry, where the contract allows 1e-4."""
import pytest
import torch

from test_gpu_parity import DEV, make_policy
from test_host_eas import reference_loss

pytestmark = pytest.mark.gpu


def setup(env_name, B=2, num_loc=20, seed=3, **kw):
    import eam_rl4co_amd as ea

    torch.manual_seed(seed)
    env = ea.get_env(env_name, generator_params=dict(num_loc=num_loc))
    td = env.reset(batch_size=[B]).to(DEV)
    pol = make_policy("am_" + env_name)
    return env, td, pol, ea.EASEmb(env, pol, **kw)


def autograd_reference(eas, s, it):
    """d loss / d logit_key by autograd through train._logp_rows on the iteration's own tours."""
    import eam_rl4co_amd as ea
    from eam_rl4co_amd import train

    pol, c = eas.policy, s.cache
    L = s.params["logit_key"].detach().clone().requires_grad_()
    dec = pol.decoder
    t = {"emb": c.node_embeddings, "K": c.view("K"), "V": c.view("V"), "L": L, "Wout": dec.pointer.project_out.weight.detach(),
         "Wctx": dec.context_embedding.project_context.weight.detach(), "gctx": c.gctx}
    if pol.env_name == "tsp":
        t["placeholder"] = dec.context_embedding.W_placeholder.detach()
    static = {k: s.td[k] for k in train._STATE_KEYS[pol.env_name]}

    def ll_of(actions, nrep):
        return train._logp_rows(pol.env_name, t, static, actions, nrep, True, dec.num_heads, pol.temperature, pol.tanh_clipping).sum(1)

    ll = ea.unbatchify(ll_of(it["actions"], s.S), (s.n_aug, s.S))                      # [B, n_aug, S]
    reward = ea.unbatchify(it["reward"], (s.n_aug, s.S))
    inc = it["inc_actions"] is not None
    if inc:
        ll = torch.cat((ll, ea.unbatchify(ll_of(it["inc_actions"], 1), s.n_aug)[..., None]), -1)
        reward = torch.cat((reward, ea.unbatchify(it["inc_reward"], s.n_aug)[..., None]), -1)
    (g,) = torch.autograd.grad(reference_loss(ll, reward, eas.baseline, eas.eas_lambda, inc), L)
    return g


@pytest.mark.parametrize("env_name", ["tsp", "cvrp"])
@pytest.mark.parametrize("incumbent", [False, True])
def test_one_iterations_logit_key_gradient(env_name, incumbent):
    env, td, pol, eas = setup(env_name)
    s = eas.begin(td, seed=7)
    assert s.fast and s.Ba == 16
    if incumbent:
        eas.step(s)
    it = eas.iteration(s, general=False)
    assert (it["inc_actions"] is not None) == incumbent
    fast = it["grads"]["logit_key"].clone()
    ref = autograd_reference(eas, s, it)
    tol = 1e-4 * float(ref.abs().max())
    err = float((fast - ref).abs().max())
    gen = eas.iteration(s, general=True, rollout=it["rollout"])["grads"]["logit_key"]
    err_gen = float((gen - fast).abs().max())
    print(f"EAS {env_name} incumbent={incumbent} max|ref| {float(ref.abs().max()):.3e} fast-ref {err:.3e} general-fast {err_gen:.3e} tol {tol:.3e}")
    assert float(ref.abs().max()) > 0 and err <= tol
    assert err_gen <= tol


def check_search(env, td, pol, eas):
    before = {k: v.clone() for k, v in pol.state_dict().items()}
    flags = [p.requires_grad for p in pol.parameters()]
    out = eas.search(td, max_iters=4, seed=7)
    best, mr = out["best_solutions"], out["max_reward"]
    assert best.dtype == torch.int64 and best.shape[0] == td.shape[0] and mr.dtype == torch.float32 and mr.shape == (td.shape[0],)
    env.check_solution_validity(td, best)
    assert torch.equal(env.get_reward(td, best), mr)
    first = eas.search(td, max_iters=1, seed=7)["max_reward"]
    assert (mr >= first).all(), (mr, first)
    assert all(torch.equal(v, before[k]) for k, v in pol.state_dict().items())
    assert [p.requires_grad for p in pol.parameters()] == flags


@pytest.mark.parametrize("env_name", ["tsp", "cvrp"])
def test_search_keeps_valid_incumbents_and_leaves_the_policy_alone(env_name):
    check_search(*setup(env_name))


@pytest.mark.parametrize("env_name", ["tsp", "cvrp"])
def test_search_over_all_three_cache_keys_takes_the_general_path(env_name):
    env, td, pol, eas = setup(env_name, eas_emb_cache_keys=["logit_key", "glimpse_key", "glimpse_val"])
    assert not eas.begin(td).fast
    check_search(env, td, pol, eas)


def test_a_113_node_instance_takes_the_general_path():
    env, td, pol, eas = setup("tsp", B=1, num_loc=113, augment_size=2, augment_dihedral=False)
    s = eas.begin(td, seed=7)
    assert not s.fast and s.M == 113 and s.Ba == 2
    out = eas.search(td, max_iters=1, seed=7)
    env.check_solution_validity(td, out["best_solutions"])
    assert sorted(out["best_solutions"][0].tolist()) == list(range(113))
    assert torch.equal(env.get_reward(td, out["best_solutions"]), out["max_reward"])
