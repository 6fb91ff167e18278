"""gym_auv_amd — MI355X-native batched implementation of gym-auv's step() hot path
(vessel dynamics -> LiDAR sweep -> path-following / collision reward), behind the
reference's gym.Env-style surface.  See DESIGN.md.

Importing this package does not touch the GPU or the HIP library; importing
`gym_auv_amd.batched_env` does (and fails loudly if libauv_hip.so is missing).
"""
from .config import Config, EpisodeConfig, SimulationConfig, VesselConfig, effective_reference_config  # noqa: F401
from .worldspec import WorldSpec, MoverSpec  # noqa: F401

__version__ = "0.1.0"


def __getattr__(name):
    # FusedPPOUpdate loads the HIP library: resolved on first use, so that importing the package still does not
    if name == "FusedPPOUpdate":
        from .ppo_update import FusedPPOUpdate
        return FusedPPOUpdate
    # PolicyPopulation: a policy per group of environments (population.py; its NumPy mirrors need no library)
    if name == "PolicyPopulation":
        from .population import PolicyPopulation
        return PolicyPopulation
    # RunningNorm: running observation / reward normalisation for the fused rollout (normalize.py; the library is loaded by its launches)
    if name == "RunningNorm":
        from .normalize import RunningNorm
        return RunningNorm
    raise AttributeError("module %r has no attribute %r" % (__name__, name))
