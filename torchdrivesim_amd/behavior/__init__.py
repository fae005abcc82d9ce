"""NPC behaviours that feed `Simulator.step` and the initial scene (reference torchdrivesim/behavior/): log replay, and the lanelet-based
random initialisation (`heuristic_initialize`, batched as `heuristic_initialize_batch`: one kernel launch).  The reference's IAI client (an
HTTP service) is outside the hot path and not provided; the reactive controller here is `LaneFollowingNPCController`: NPCs that follow the lane
graph at the speed the Intelligent Driver Model gives them, one kernel launch per step."""
from torchdrivesim_amd.behavior.common import InitializationFailedError
from torchdrivesim_amd.behavior.heuristic import heuristic_initialize, heuristic_initialize_batch
from torchdrivesim_amd.behavior.lane_follow import LaneFollowingNPCController
from torchdrivesim_amd.behavior.replay import ReplayController, interaction_replay

__all__ = ['InitializationFailedError', 'LaneFollowingNPCController', 'ReplayController', 'interaction_replay', 'heuristic_initialize', 'heuristic_initialize_batch']
