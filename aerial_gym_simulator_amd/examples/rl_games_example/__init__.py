"""aerial_gym/examples/rl_games_example of the reference: the inference class its closed-loop example and ROS node import."""
