"""gym_pbn_amd -- MI355X-native vectorised Probabilistic Boolean Network simulator.

Drop-in for the async-update hot path of gym-PBN (``gym_PBN/envs``): bit-packed
env states in HBM, hand-written gfx950 HIP kernels (libpbnsim.so, C ABI in
``include/pbn_abi.h``), reached through ctypes.

Importing the network/descriptor helpers needs no GPU; anything that steps
envs loads libpbnsim and fails loudly if it is missing.
"""

from .network import (  # noqa: F401
    KIND_PREDICTOR_MIX,
    KIND_PROB_TABLE,
    PredictorNetwork,
    TruthTableNetwork,
    load_network,
    synthetic_truth_table_pbn,
)

__version__ = "0.1.0"


def __getattr__(name):
    # lazy: loading libpbnsim (and torch) only when a device object is needed
    if name in ("Net", "EnvConfig", "PBNBatch", "pack_bits", "unpack_bits"):
        from . import batch

        return getattr(batch, name)
    if name in ("Graph", "PBN", "PBNTargetEnv", "PBNTargetMultiEnv", "VecPBNTargetMultiEnv", "VecPBNEnv", "PBNEnv",
                "state_to_idx"):
        from . import envs

        return getattr(envs, name)
    if name in ("find_attractors", "AttractorResult", "ReachSet", "cube_cover", "host_unstable"):
        from . import attractors

        return getattr(attractors, name)
    if name == "StateSet":
        from .stateset import StateSet

        return StateSet
    if name in ("StateCensus", "CensusResult", "statistical_attractors"):
        from . import census

        return getattr(census, name)
    if name in ("TransitionGraph", "host_edge_mass"):
        from . import transition

        return getattr(transition, name)
    if name in ("ControlProblem", "ControlSolution", "host_backup", "host_expect"):
        from . import control

        return getattr(control, name)
    if name in ("Absorption", "AbsorptionResult", "host_absorb_sweep"):
        from . import absorption

        return getattr(absorption, name)
    if name in ("MultiFlipProblem", "MultiFlipSolution", "host_multiflip_max", "host_multiflip_arrival"):
        from . import multiflip

        return getattr(multiflip, name)
    if name in ("TorchVecPBNEnv", "TorchVecPBNTargetMultiEnv", "TorchVecPBNTargetMultiSetEnv"):
        from . import torch_env

        return getattr(torch_env, name)
    if name in ("TorchVecPBNSampledDataEnv", "TorchVecPBNSelfTriggeringEnv", "stop_thresholds", "gamma_powers",
                "decode_discrete"):
        from . import macro_env

        return getattr(macro_env, name)
    if name == "make":
        from .registry import make

        return make
    raise AttributeError(name)
