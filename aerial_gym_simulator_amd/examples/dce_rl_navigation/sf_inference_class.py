"""NN_Inference_Class with the reference's surface (aerial_gym/examples/dce_rl_navigation/sf_inference_class.py:27-101): the same
implementation as sim2real/nn_inference_class.py Sim2RealInferenceClass (the reference's two files differ in the observation key
alone, and get_action here reads either)."""
from ...utils.policy import SampleFactoryInference


class NN_Inference_Class(SampleFactoryInference):
    pass
