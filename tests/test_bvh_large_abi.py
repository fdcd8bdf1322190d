"""The C ABI of the global-memory LBVH build (csrc/agx_scene_large.hip; ABI 21): argument refusals by message, the scratch-size
function, the mirrors in _lib and the header, and the kernel's resources.  CPU only: every refused call returns before anything
touches the GPU, and the rest reads the built library."""
import ctypes as C
import os
import re

import pytest

import codeobj

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("agx_bvh_large_scratch_bytes", "agx_bvh_build_large", "agx_scene_refresh_large")
P16 = C.c_void_p(16)
CAP = 65536


def _build_large(lib, n, nt, ppo=0, mask=None, work=None, scratch=P16, nbytes=None, tri=P16, nodes=P16):
    nbytes = lib.agx_bvh_large_scratch_bytes(n, nt) if nbytes is None else nbytes
    return lib.agx_bvh_build_large(n, nt, ppo, tri, mask, nodes, work, scratch, nbytes, None)


def _refresh_large(lib, n, nt, ppo=0, mask=None, work=None, scratch=P16, nbytes=None, tri_local=P16):
    nbytes = lib.agx_bvh_large_scratch_bytes(n, nt) if nbytes is None else nbytes
    return lib.agx_scene_refresh_large(n, nt, 1, tri_local, P16, P16, None, ppo, mask, P16, None, P16, work, scratch, nbytes, None)


def test_large_build_refuses_bad_arguments_by_message():
    from aerial_gym_simulator_amd import _lib

    lib = _lib.load()
    err = lambda: lib.agx_last_error().decode()  # noqa: E731
    for call in (_build_large, _refresh_large):
        for nt in (1, CAP + 1):
            assert call(lib, 4, nt, nbytes=1 << 30) == -1
            assert f"num_tris {nt} " in err() and "65536" in err()
        need = lib.agx_bvh_large_scratch_bytes(4, 4097)
        assert call(lib, 4, 4097, nbytes=need - 1) == -1                        # a short scratch buffer: both byte counts
        assert str(need - 1) in err() and str(need) in err()
        assert call(lib, 4, 4097, scratch=None) == -1 and "scratch" in err()     # null scratch
        assert call(lib, 4, 4097, mask=P16, work=None) == -1 and "work" in err()  # a masked call without the work list
        assert call(lib, 4, 4097, ppo=12 | 0x20000000) == -1                     # 4097 is not a multiple of 12
        assert call(lib, 0, 4097, nbytes=1 << 30) == -1
    assert _build_large(lib, 4, 4097, tri=None) == -1 and "null buffer" in err()
    assert _build_large(lib, 4, 4097, nodes=None) == -1 and "null buffer" in err()
    assert _refresh_large(lib, 4, 4097, tri_local=None) == -1 and "null buffer" in err()


def test_old_entry_points_keep_the_lds_cap():
    from aerial_gym_simulator_amd import _lib

    lib = _lib.load()
    for ppo in (0, 12 | 0x30000000):
        assert lib.agx_bvh_build(4, 2945, ppo, P16, None, P16, None, None) == -1
        assert b"num_tris 2945" in lib.agx_last_error()
    assert lib.agx_scene_refresh(4, 2945, 1, P16, P16, P16, None, 0, P16, P16, None, P16, P16, None) == -1
    assert b"num_tris 2945" in lib.agx_last_error()


def test_scratch_bytes_is_positive_monotone_and_stops_growing_with_the_env_count():
    from aerial_gym_simulator_amd import _lib

    f = _lib.load().agx_bvh_large_scratch_bytes
    sizes = (2, 3, 24, 511, 513, 2945, 4096, 4097, 8193, 32768, 32769, CAP)
    envs = (1, 2, 5, 64, 255, 256, 257, 1024, 8192)
    for n in envs:
        row = [f(n, nt) for nt in sizes]
        assert all(b > 0 for b in row) and row == sorted(row), (n, row)
    for nt in sizes:
        col = [f(n, nt) for n in envs]
        assert col == sorted(col), (nt, col)
        assert f(256, nt) == f(257, nt) == f(8192, nt) == f(1 << 20, nt) and f(255, nt) < f(256, nt)  # one slab per resident workgroup
        assert f(1, nt) <= 64 * nt + 1024                                                              # a slab: at most 64 B per triangle
    assert f(1 << 20, CAP) < 1 << 30                                                                   # below 1 GiB at the cap
    assert f(4, 1) == 0 and f(4, CAP + 1) == 0 and f(0, 24) == 0                                        # what the build refuses


def test_header_lib_and_symbols_agree_on_the_new_entry_points():
    from aerial_gym_simulator_amd import _build, _lib

    header = open(os.path.join(ROOT, "include", "aerial_gym_hip.h")).read()
    assert int(re.search(r"#define AGX_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION >= 21
    assert _lib.load().agx_abi_version() == _lib.ABI_VERSION
    for name in NEW:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(_lib.load(), name)
    assert "asset_manager.py:51-71" in header[header.index("agx_bvh_large_scratch_bytes") - 2500: header.index("agx_bvh_large_scratch_bytes")]
    assert "agx_scene_large.hip" in _build.SOURCES


@pytest.mark.skipif(not codeobj.tools_available(), reason="objcopy / ROCm LLVM tools not found")
def test_large_build_kernel_has_no_spills_and_no_scratch():
    from aerial_gym_simulator_amd import _build

    meta = {n: r for n, r in codeobj.kernel_metadata(_build.LIB_PATH).items() if "k_bvh_build_large" in n}
    assert len(meta) == 1, list(meta)
    (rec,) = meta.values()
    assert rec["vgpr_spill_count"] == 0 and rec["private_segment_fixed_size"] == 0, rec
    assert rec["group_segment_fixed_size"] <= 64 * 1024, rec  # the sort tile: several workgroups fit a CU's LDS


def test_scene_manager_selects_the_large_build_and_refuses_above_its_cap():
    """host side, no device: three 13-link trees (5580 triangles) built -> large_build; the same scene above 65536 triangles and a box
    scene of 5462 boxes (65544 triangles) raise ValueError; small scenes keep the LDS builders unless forced"""
    import aerial_gym_simulator_amd  # noqa: F401
    from aerial_gym_simulator_amd.config import asset_config as A
    from aerial_gym_simulator_amd.config.env_config import EnvWithObstaclesCfg, ForestEnvCfg
    from aerial_gym_simulator_amd.env_manager.scene_manager import SceneManager

    def forest(count):
        class trees(A.tree_asset_params):
            num_assets = count
            asset_folder = os.path.join(ROOT, "tests", "fixtures", "assets", "trees13")

        class Cfg(ForestEnvCfg):
            class env_config:
                include_asset_type = {"trees": True, "objects": True, "bottom_wall": True}
                asset_type_to_dict_map = {"trees": trees, "objects": A.object_asset_params, "bottom_wall": A.bottom_wall}

        return Cfg

    assert SceneManager.MAX_TRIS_PER_ENV == 2944 and SceneManager.MAX_TRIS_PER_ENV_LARGE == CAP
    one, three = SceneManager(forest(1), 2, "cpu", None), SceneManager(forest(3), 2, "cpu", None)
    assert one.num_tris == 2148 and not one.large_build
    assert three.num_tris == 5580 and three.large_build
    assert SceneManager(forest(1), 2, "cpu", None, force_large_build=True).large_build
    with pytest.raises(ValueError, match="65536.*largest assets"):
        SceneManager(forest(38), 1, "cpu", None)  # 12 + 38 * 1716 + 420 = 65640

    class many_boxes(A.object_asset_params):
        num_assets = 5462

    class Boxes(EnvWithObstaclesCfg):
        class env_config:
            include_asset_type = {"objects": True}
            asset_type_to_dict_map = {"objects": many_boxes}

    with pytest.raises(ValueError, match="65544 triangles"):
        SceneManager(Boxes, 1, "cpu", None)
    boxes = SceneManager(EnvWithObstaclesCfg, 2, "cpu", None)
    assert not boxes.large_build and SceneManager(EnvWithObstaclesCfg, 2, "cpu", None, force_large_build=True).large_build
