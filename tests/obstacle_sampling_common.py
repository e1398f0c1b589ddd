"""Shared by tests/test_obstacle_sampling.py and tests/test_obstacle_sampling_gpu.py: the yardstick of
a sampled choice -- the inverse CDF of oracle.model's branch_eval at the recorded pre-step state under
bmpc.rng's draw.  The scenes and their host steps are tests/scene_common.py's."""
import numpy as np

from bmpc import rng

MARGIN = 1e-9          # the project's host-versus-NumPy scene bar (tests/test_env_host.py)
MAX_LEFT_OUT = 0.01    # at most 1 % of the decisions may lie within MARGIN of a partial sum


def expected_choice(p, u):
    """(choice, sure): bmpc.rng's inverse CDF of probabilities p [..., m] at u [...], and whether u
    keeps MARGIN from every partial sum that separates two policies."""
    choice, cum = rng.inverse_cdf(p, u)
    return choice, np.abs(np.asarray(u)[..., None] - cum[..., :-1]).min(-1) >= MARGIN


def check_choices(sc, smp, choices, pre, ego_base=0):
    """The rule of every sampled choice of a run.  choices [T][B]: the scene row's policy index after
    each step; pre [T]: (pol, x, z) the policies in force before the step and the step's pre-step
    state (its x / z outputs) -- needed at epoch starts only (None elsewhere).  Epoch starts equal the
    inverse CDF of the oracle's p under bmpc.rng's u unless u lies within MARGIN of a partial sum (at
    most MAX_LEFT_OUT of them may); inside an epoch the choice is the epoch's first.  Returns the
    number of compared draws."""
    T, B = np.asarray(choices).shape
    left_out = draws = 0
    for t in range(T):
        if t % smp.hold:
            np.testing.assert_array_equal(choices[t], choices[t - t % smp.hold], err_msg=f"step {t} inside an epoch")
            continue
        pol, x, z = pre[t]
        u = rng.obstacle_uniform(smp.seed, ego_base + np.arange(B), t // smp.hold)
        p = np.stack([sc.oracle_p(pol, e, x[e], z[e]) for e in range(B)])
        want, sure = expected_choice(p, u)
        draws += B
        left_out += int((~sure).sum())
        np.testing.assert_array_equal(np.asarray(choices[t])[sure], want[sure], err_msg=f"epoch start {t}")
    assert left_out <= MAX_LEFT_OUT * draws, (left_out, draws)
    return draws - left_out
