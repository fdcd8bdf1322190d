"""forest_env with SEVERAL trees per env (the reference's forest: 13-link cylinder trees, 1716 triangles each).  Three of them,
35 objects and the floor are 5580 triangles per env: above the 2944 the LDS-resident tree build takes, so the scene goes through
the global-memory build (SceneManager.large_build, agx_scene_refresh_large; up to 65536 triangles per env).

Trees come from $AERIAL_GYM_RESOURCES/models/environment_assets/trees when that is set, else from the synthetic 13-link tree of
tests/fixtures/assets/trees13.  AGX_FOREST_TREES sets the number of trees per env."""
import os

import torch

import aerial_gym_simulator_amd  # noqa: F401
from aerial_gym_simulator_amd.config import asset_config as A
from aerial_gym_simulator_amd.config.env_config import ForestEnvCfg
from aerial_gym_simulator_amd.registry.env_registry import env_config_registry
from aerial_gym_simulator_amd.sim.sim_builder import SimBuilder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def forest_cfg(num_trees):
    folder = A.tree_asset_params.asset_folder
    if not os.environ.get("AERIAL_GYM_RESOURCES") or not os.path.isdir(folder):
        folder = os.path.join(ROOT, "tests", "fixtures", "assets", "trees13")

    class trees(A.tree_asset_params):
        num_assets = num_trees
        asset_folder = folder

    class Cfg(ForestEnvCfg):
        class env_config:
            include_asset_type = {"trees": True, "objects": True, "bottom_wall": True}
            asset_type_to_dict_map = {"trees": trees, "objects": A.object_asset_params, "bottom_wall": A.bottom_wall}

    return Cfg


if __name__ == "__main__":
    env_config_registry.register("forest_env_several_trees", forest_cfg(int(os.environ.get("AGX_FOREST_TREES", 3))))
    env = SimBuilder().build_env(sim_name="base_sim", env_name="forest_env_several_trees", robot_name="base_quadrotor_with_camera_64x48",
                                 controller_name="lee_velocity_control", args=None, device="cuda:0", num_envs=16, headless=True, use_warp=True)
    sc = env.scene
    print(f"{sc.num_tris} triangles per env in {sc.num_prims} pieces; large build: {sc.large_build}"
          + (f", {sc.bvh_scratch.numel() / 2**20:.1f} MiB of build scratch" if sc.large_build else ""))
    actions = torch.zeros((env.num_envs, 4), device="cuda:0")
    actions[:, 0] = 0.5  # fly along +x, into the trees
    env.reset()
    g = env.get_obs()
    for i in range(int(os.environ.get("AGX_EXAMPLE_STEPS", 1000))):
        env.step(actions=actions)
        env.post_reward_calculation_step()  # resets the crashed envs: their scenes are rebuilt
        if i % 100 == 99:
            print(f"step {i + 1}: crashes {int(g['crashes'].sum())}, mean depth {float(g['depth_range_pixels'].mean()):.3f}, "
                  f"tree pixels {int((g['segmentation_pixels'] >= 100).sum())}")
