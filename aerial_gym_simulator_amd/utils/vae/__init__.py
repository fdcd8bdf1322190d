"""The reference's aerial_gym/utils/vae: the depth-image encoder of the navigation task (vae_image_encoder.py)."""
