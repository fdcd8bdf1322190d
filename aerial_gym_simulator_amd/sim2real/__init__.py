"""aerial_gym/sim2real of the reference: the inference class its sample-factory deployment scripts import."""
