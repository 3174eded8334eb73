"""MidlevelAgent.calibrate_ideal_constraints: the calibration of the frame's records on the ideal
rollout those records were built from, through the eager generators and predict_and_constrain,
against the engine-level oracle (engine.ideal_rollout + engine.risk_quantile) run with the
agent's seed rule, previous moments and source cells.  Everything is compared for equality."""
import numpy as np
import pytest
import torch

from oracle import ccmpc_oracle as orc

pytestmark = pytest.mark.gpu

N_IDEAL = 4099


class Params:
    def __init__(self, O, K, frame):
        self.O, self.K, self.frame = O, np.asarray(K), frame


def _oracle(agent, frame, prev_frame, K, T, kind, R=None, eps=None):
    """(risk.calibration_report of the materialised rollout's calibration, its RiskQuantile, the
    records as [C, P', 128] bytes), from the agent's saved state."""
    from ccmpc import engine, risk
    dev = agent.device
    pm, pc, prev_K, _ = agent._moments[prev_frame]
    pm, pc = torch.as_tensor(pm, device=dev), torch.as_tensor(pc, device=dev)
    src = torch.as_tensor(agent._src_cells_host(prev_K, K), device=dev)
    seed = (agent.seed * 1_000_003 + frame) & (2**63 - 1)
    store, status = engine.ideal_rollout(pm, pc, src, T, agent.n_ideal, seed=seed)
    rec, rec_kind, rec_T = agent._last_rec
    assert rec_kind == kind and rec_T == T
    C = sum(K)
    rec = engine._rec_bytes(rec, kind, C)
    counts = [agent.n_ideal] * C
    ph = agent.prediction_horizon
    eps = risk.EPS_TOTAL if eps is None else eps
    allow = risk.allow_counts(counts, K, ph, eps)
    quant = engine.risk_quantile(store, rec, kind, allow=allow,
                                 R=agent.R if R is None else R, T=T)
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0] * C
    report = risk.calibration_report(quant, engine.record_fields(rec, kind), counts, K, ph, eps)
    return report, quant, rec


def _same_report(got, want):
    assert got.keys() == want.keys()
    for k, w in want.items():
        g = got[k]
        if isinstance(w, np.ndarray):
            assert g.shape == w.shape and g.dtype == w.dtype, k
            assert np.array_equal(g, w, equal_nan=w.dtype.kind == "f"), k
        else:
            assert g == w, k


def _checks(agent, frame, prev_frame, K, T, kind):
    from ccmpc import engine
    before = (agent._last_rec, agent._audit_src, agent._ideal_audit_src, agent.last_records)
    bytes_before = engine._rec_bytes(agent._last_rec[0], kind, sum(K)).clone()
    got = agent.calibrate_ideal_constraints()
    assert isinstance(got, dict)                                 # no mode: the report alone
    want, quant, rec = _oracle(agent, frame, prev_frame, K, T, kind)
    _same_report(got, want)
    assert got["counts"].tolist() == [N_IDEAL] * sum(K)
    assert (got["status"] == 0).any()                            # not vacuous
    # a larger budget and another radius reach the kernel
    wide = agent.calibrate_ideal_constraints(R=2 * agent.R, eps=0.8)
    _same_report(wide, _oracle(agent, frame, prev_frame, K, T, kind, R=2 * agent.R, eps=0.8)[0])
    assert wide["allow"].max() > 0 and np.all(wide["allow"] >= got["allow"])
    # with a mode: records in the layout the planning QP reads, the frame's own left alone
    for mode in ("tighten", "replace"):
        report, cal_rec = agent.calibrate_ideal_constraints(mode=mode)
        _same_report(report, want)
        assert cal_rec.dtype == torch.uint8 and cal_rec.is_contiguous()
        assert cal_rec.shape == rec.shape and cal_rec.device == rec.device
        assert torch.equal(cal_rec, engine.calibrated_records(rec, kind, quant, mode))
    assert not torch.equal(cal_rec, rec)                         # "replace" moved an offset
    with pytest.raises(ValueError):
        agent.calibrate_ideal_constraints(mode="loosen")
    after = (agent._last_rec, agent._audit_src, agent._ideal_audit_src, agent.last_records)
    assert all(a is b for a, b in zip(before, after))            # no planner state changed
    assert torch.equal(engine._rec_bytes(agent._last_rec[0], kind, sum(K)), bytes_before)


def _eager_agent(gpu, scene_seed, seed):
    from ccmpc import ovehicle, planner, synthetic
    T = 8
    ov_cells, ref, pasts = synthetic.scene(scene_seed, O=2, N=2500, T=T)
    K = [len(c) for c in ov_cells]
    ovs = ovehicle.scene_from_positions(ov_cells, pasts, device=gpu)
    agent = planner.MidlevelAgent(prediction_horizon=T, n_ideal=N_IDEAL, seed=seed, device=gpu)
    return agent, ovs, K, ref, T


def test_eager_minkowski_generator(gpu):
    from ccmpc import mpc
    agent, ovs, K, ref, T = _eager_agent(gpu, 44, 5)
    eps = orc.eps_ura_matrix(K)
    with pytest.raises(RuntimeError):
        agent.calibrate_ideal_constraints()                      # no frame yet
    agent.compute_obstacle_constraints_GMM_Minkowski_idealprediction(
        Params(len(K), K, 200), ovs, None, None, None, eps, None, T, ref)
    with pytest.raises(RuntimeError):
        agent.calibrate_ideal_constraints()                      # Tsh == ph: the sampled scene
    agent.compute_obstacle_constraints_GMM_Minkowski_idealprediction(
        Params(len(K), K, 210), ovs, None, None, None, eps, None, T - 1, ref)
    _checks(agent, 210, 200, K, T - 1, mpc.REC_HALFSPACE)
    # a later frame that is not an ideal-rollout frame forgets it
    agent.compute_obstacle_constraints_GMM_affine(
        Params(len(K), K, 220), ovs, None, None, None, eps, None, T, ref)
    with pytest.raises(RuntimeError):
        agent.calibrate_ideal_constraints()


def test_eager_affine_tangent_generator(gpu):
    from ccmpc import mpc
    agent, ovs, K, ref, T = _eager_agent(gpu, 61, 6)
    eps = orc.eps_ura_matrix(K)
    x_init = np.array([ref[0][0] - 4.0, ref[0][1] - 0.5, 0.0, 5.0])
    p1, p2 = Params(len(K), K, 300), Params(len(K), K, 310)
    p1.x_init = p2.x_init = x_init
    agent.compute_obstacle_constraints_GMM_affine_scale_ideal(
        p1, ovs, None, None, None, eps, None, T, ref)
    with pytest.raises(RuntimeError):
        agent.calibrate_ideal_constraints()
    agent.compute_obstacle_constraints_GMM_affine_scale_ideal(
        p2, ovs, None, None, None, eps, None, T - 1, ref + np.array([2.0, 0.25]))
    _checks(agent, 310, 300, K, T - 1, mpc.REC_AFFINE)


def test_predict_and_constrain(gpu):
    from ccmpc import episode, mpc
    rep = episode.EpisodeReplay(O=2, N=3000, ph=8, n_ideal=N_IDEAL, receding_steps=1, seed=5,
                                device=gpu)
    agent, ph = rep.agent, 8
    assert agent.n_ideal == N_IDEAL
    K = [int(np.count_nonzero(rep.pmf[o] > 0.1)) for o in range(rep.O)]
    eps = np.full((rep.O, max(K)), 0.05 / rep.O)
    ref = rep.ref_traj(0)
    sampler = dict(init_state=rep.init, latent_pmf=rep.pmf, gmm=rep.gmm, N=rep.N,
                   seed=rep.seed * 7919)
    agent.predict_and_constrain(episode.Params(rep.O, K, 0), sampler, eps, ph, ref, rep.minpos,
                                rep.pasts)
    with pytest.raises(RuntimeError):
        agent.calibrate_ideal_constraints()                      # Tsh == ph
    assert isinstance(agent.calibrate_constraints(), dict)       # ... is calibrate_constraints'
    T = ph - 1
    ref = rep.ref_traj(10)
    sampler["seed"] = rep.seed * 7919 + 10
    agent.predict_and_constrain(episode.Params(rep.O, K, 10), sampler, eps, T, ref[:T],
                                rep.minpos, rep.pasts)
    _checks(agent, 10, 0, K, T, mpc.REC_HALFSPACE)
    # the neighbouring method on the same frame still refuses, and names this one
    with pytest.raises(RuntimeError, match="calibrate_ideal_constraints"):
        agent.calibrate_constraints()
