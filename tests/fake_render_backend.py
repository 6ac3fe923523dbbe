"""Stand-in with BatchedSim's render surface for CPU tests of BalanceVecEnv's rendering logic (tests only): the oracle plays
the simulator and the numpy reference (tests/ref_render.py) plays the render kernel."""
import numpy as np

from tests import ref_render
from tests.fake_backend import OracleSim


class OracleRenderSim(OracleSim):
    """`camera`: the camera used when render() is given none (small images keep the numpy reference fast)"""

    def __init__(self, env_id, n, camera=None, **kw):
        super().__init__(env_id, n, **kw)
        self.env_id, self.camera = env_id, camera
        self.rendered = []  # env_ids of every render() call

    def render(self, env_ids=None, camera=None):
        ids = np.arange(self.n) if env_ids is None else np.asarray(env_ids)
        self.rendered.append(ids.tolist())
        qpos = self.o.get_state()[0]
        block = self.env_id.startswith("Env03")
        return np.stack([ref_render.render(qpos[i], block, camera or self.camera)[0] for i in ids])
