"""aerial_gym/examples/dce_rl_navigation of the reference: the inference class its navigation example imports."""
