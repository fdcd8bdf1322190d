"""Sim2RealInferenceClass with the reference's surface (aerial_gym/sim2real/nn_inference_class.py:27-101): a sample-factory actor
with a GRU core, `Sim2RealInferenceClass(num_envs, num_actions, num_obs, cfg)`, `get_action(obs_dict)`, `reset(env_ids)`,
`rnn_states`.  Built on RecurrentActor: on a HIP device a get_action is one launch of the library's fused kernel
(csrc/agx_policy.hip k_recurrent_act); sample-factory itself is not needed.  utils/policy.py SampleFactoryInference states the
differences."""
from ..utils.policy import SampleFactoryInference


class Sim2RealInferenceClass(SampleFactoryInference):
    pass
