"""GPU: the EAS-Lay search (eam_rl4co_amd/search.py) -- one iteration's four layer gradients (one eamrl_eas_layer_backward launch
on the rollout's own log-probs and heads) against torch autograd through the PyTorch re-evaluation (train._logp_rows) of the same
tours, with the layer as an nn.Module between the heads and project_out and the loss as the reference writes it
(zoo/eas/search.py:223-241; test_host_eas.reference_loss); and whole searches: valid incumbents whose reward is max_reward bit for
bit and never decreases, a layer that has moved, an untouched policy, equal results for equal seeds.
Tolerance of the gradients: the native-versus-autograd contract of tests/test_gpu_eas.py, atol = 1e-4 max|ref| per gradient."""
import pytest
import torch

from test_gpu_parity import DEV, make_policy
from test_host_eas import reference_loss

pytestmark = pytest.mark.gpu

PARAMS = ("W1", "b1", "W2", "b2")


def setup(env_name, B=2, num_loc=20, seed=3, **kw):
    import eam_rl4co_amd as ea

    torch.manual_seed(seed)
    env = ea.get_env(env_name, generator_params=dict(num_loc=num_loc))
    td = env.reset(batch_size=[B]).to(DEV)
    pol = make_policy("am_" + env_name)
    return env, td, pol, ea.EASLay(env, pol, **kw)


class Layer(torch.nn.Module):
    """EASLayerNet (zoo/eas/nn.py:5-30) on rows in (s b) order: row r uses the weights of instance r % N."""

    def __init__(self, W1, b1, W2, b2):
        super().__init__()
        self.W1, self.b1, self.W2, self.b2 = (torch.nn.Parameter(x.clone()) for x in (W1, b1, W2, b2))

    def forward(self, h):                   # h [R, T, E] -> the heads with the residual added
        i = torch.arange(h.shape[0], device=h.device) % self.W1.shape[0]
        a = torch.relu(torch.bmm(h, self.W1[i]) + self.b1[i][:, None, :])
        return h + torch.bmm(a, self.W2[i]) + self.b2[i][:, None, :]


def autograd_reference(eas, s, it):
    """d loss / d (W1, b1, W2, b2) in the reference's shapes by autograd through train._logp_rows on the iteration's own tours."""
    import eam_rl4co_amd as ea
    from eam_rl4co_amd import ops, train

    pol, c = eas.policy, s.cache
    layer = Layer(ops.unpack_eas_layer(s.params["W1"].detach()), s.params["b1"].detach(), ops.unpack_eas_layer(s.params["W2"].detach()),
                  s.params["b2"].detach())
    dec = pol.decoder
    t = {"emb": c.node_embeddings, "K": c.view("K"), "V": c.view("V"), "L": c.view("L"), "Wout": dec.pointer.project_out.weight.detach(),
         "Wctx": dec.context_embedding.project_context.weight.detach(), "gctx": c.gctx, "eas_layer": layer}
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
    grads = torch.autograd.grad(reference_loss(ll, reward, eas.baseline, eas.eas_lambda, inc), [getattr(layer, n) for n in PARAMS],
                                allow_unused=True)
    return {n: (g if g is not None else torch.zeros_like(getattr(layer, n))) for n, g in zip(PARAMS, grads)}


def native_grads(it):
    from eam_rl4co_amd import ops

    g = it["grads"]
    return {"W1": ops.unpack_eas_layer(g["W1"]), "b1": g["b1"], "W2": ops.unpack_eas_layer(g["W2"]), "b2": g["b2"]}


@pytest.mark.parametrize("env_name", ["tsp", "cvrp"])
@pytest.mark.parametrize("incumbent", [False, True])
def test_one_iterations_layer_gradients(env_name, incumbent):
    env, td, pol, eas = setup(env_name)
    s = eas.begin(td, seed=7)
    assert s.Ba == 16 and not s.fast
    assert not s.params["W2"].detach().any() and not s.params["b2"].detach().any() and float(s.params["W1"].detach().abs().max()) > 0
    it0 = eas.iteration(s)
    assert it0["inc_actions"] is None
    assert (it0["grads"]["W1"] == 0).all() and (it0["grads"]["b1"] == 0).all()          # W2 = 0: nothing reaches the first layer
    eas.step(s)
    eas.step(s)                             # two steps: every parameter has moved, the incumbent exists
    if not incumbent:
        s.best = None                       # the same adapted layer, an iteration without the imitation term
    it = eas.iteration(s)
    assert (it["inc_actions"] is not None) == incumbent
    if incumbent:
        R = it["inc_actions"].shape[0]
        assert R == s.Ba and it["rollout"][0].shape[0] == (s.S + 1) * s.Ba
        w = min(s.best.shape[1], it["inc_actions"].shape[1])
        assert torch.equal(it["inc_actions"][:, :w], s.best.repeat(s.n_aug, 1)[:, :w])      # the forced row is the incumbent
    got, ref = native_grads(it), autograd_reference(eas, s, it)
    for n in PARAMS:
        top = float(ref[n].abs().max())
        err = float((got[n] - ref[n]).abs().max())
        print(f"EASLAY {env_name} incumbent={incumbent} d{n}: max|ref| {top:.3e} kernel-autograd {err:.3e} tol {1e-4 * top:.3e}")
        assert top > 0 and err <= 1e-4 * top


@pytest.mark.parametrize("env_name", ["tsp", "cvrp"])
def test_search_keeps_valid_incumbents_moves_the_layer_and_leaves_the_policy_alone(env_name):
    env, td, pol, eas = setup(env_name)
    before = {k: v.clone() for k, v in pol.state_dict().items()}
    flags = [p.requires_grad for p in pol.parameters()]
    s = eas.begin(td, seed=7)
    trace = []
    for _ in range(4):
        eas.step(s)
        trace.append(s.max_reward.clone())
        env.check_solution_validity(td, s.best)
        assert torch.equal(env.get_reward(td, s.best), s.max_reward)
    assert all(bool((b >= a).all()) for a, b in zip(trace, trace[1:]))
    assert float(s.params["W2"].detach().abs().max()) > 0
    out = eas.search(td, max_iters=4, seed=7)
    best, mr = out["best_solutions"], out["max_reward"]
    assert best.dtype == torch.int64 and best.shape[0] == td.shape[0] and mr.dtype == torch.float32 and mr.shape == (td.shape[0],)
    env.check_solution_validity(td, best)
    assert torch.equal(env.get_reward(td, best), mr)
    a = eas.search(td, max_iters=1, seed=7)["max_reward"]
    b = eas.search(td, max_iters=1, seed=7)["max_reward"]
    assert torch.equal(a, b) and (mr >= a).all()
    assert all(torch.equal(v, before[k]) for k, v in pol.state_dict().items())
    assert [p.requires_grad for p in pol.parameters()] == flags


def test_unsupported_layer_searches_name_their_limit():
    import eam_rl4co_amd as ea

    env, td, pol, eas = setup("tsp")
    with pytest.raises(NotImplementedError, match="together are not built"):
        ea.EAS(env, pol, use_eas_embedding=True, use_eas_layer=True)
    op_env = ea.get_env("op", generator_params=dict(num_loc=20))
    with pytest.raises(NotImplementedError, match="env 'op' is not built"):
        ea.EASLay(op_env, ea.AttentionModelPolicy(env_name="op").eval().to(DEV))
    with pytest.raises(NotImplementedError, match="num_parallel_runs"):
        ea.EASLay(env, pol, num_parallel_runs=2)
    big = ea.get_env("tsp", generator_params=dict(num_loc=113))
    with pytest.raises(NotImplementedError, match="above 112 nodes"):
        ea.EASLay(big, pol, augment_size=2, augment_dihedral=False).begin(big.reset(batch_size=[1]).to(DEV))
    wide = ea.get_env("cvrp", generator_params=dict(num_loc=111))          # 112 nodes, but S + 1 = 112 <= 128: supported shape
    assert ea.EASLay(wide, make_policy("am_cvrp"), augment_size=2, augment_dihedral=False).begin(wide.reset(batch_size=[1]).to(DEV)).S == 111
