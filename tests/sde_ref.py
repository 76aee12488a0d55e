"""numpy restatement of the process-noise draws of csrc/vihds_sde.hpp (noisy_step / noisy_step_vjp): the counter layout on top
of philox_ref.philox4x32_10, the Box-Muller pairs of csrc/vihds_rng.hpp.  Used by the tests as the checker."""
import numpy as np

from philox_ref import philox4x32_10

STREAM_TAG = 0x53444531  # kSdeStreamTag: the fourth counter word of the process-noise stream (the theta stream has 0)
KEY_WORD = 1 << 24  # each key word is an integer in [0, 2^24)


def counter(traj, species, step):
    """(c0, c1, c2, c3) of the draw of `species` at `step` of trajectory `traj`, and the normal's place in the block."""
    return (traj, species >> 2, step, STREAM_TAG), species & 3


def step_index(k, substeps, j):
    """The step index of sub-step j of observation interval k."""
    return k * substeps + j


def expected_draws(B, S, N, n_steps, key):
    """xi [B, S, N, n_steps] (float32) under the key (lo, hi), or per-row keys [B, 2]: species q of step c of trajectory b * S + s
    is normal q & 3 of the block at the counter (b * S + s, q >> 2, c, STREAM_TAG)."""
    key = np.broadcast_to(np.asarray(key, dtype=np.int64), (B, 2))
    assert key.min() >= 0 and key.max() < KEY_WORD
    b, s, q, c = np.meshgrid(np.arange(B), np.arange(S), np.arange(N), np.arange(n_steps), indexing="ij")
    (c0, c1, c2, c3), lane = counter(b * S + s, q, c)
    r = philox4x32_10(c0.astype(np.uint64), c1.astype(np.uint64), c2.astype(np.uint64), np.full(b.shape, c3, dtype=np.uint64),
                      key[b, 0].astype(np.uint64), key[b, 1].astype(np.uint64))
    x = np.where(lane & 2, r[2], r[0]).astype(np.float32)
    y = np.where(lane & 2, r[3], r[1]).astype(np.float32)
    u1 = np.minimum((x + np.float32(0.5)) * np.float32(2.0 ** -32), np.float32(0.99999994))
    u2 = (y + np.float32(0.5)) * np.float32(2.0 ** -32)
    rad = np.sqrt(np.float32(-2.0) * np.log(u1.astype(np.float64)))
    ang = 2.0 * np.pi * u2.astype(np.float64)
    return np.where(lane & 1, rad * np.sin(ang), rad * np.cos(ang)).astype(np.float32)
