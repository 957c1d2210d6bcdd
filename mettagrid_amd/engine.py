"""Python host side of the MI355X MettaGrid step engine: ctypes binding of libmgx (include/mgx.h) plus mirrors of
the reference's Python-visible interface.

* ``BatchedMettaGrid`` — E envs per engine, buffers ``[E*A, T, 3]`` etc. resident in HBM (torch tensors are used
  only as device-memory handles).
* ``MettaGrid`` — same constructor, methods and error behaviour as the reference's pybind class
  ``mettagrid.mettagrid_c.MettaGrid`` (/root/reference/cpp/bindings/mettagrid_py.cpp:242-397, type stub
  python/src/mettagrid/mettagrid_c.pyi:752-806) for ONE env, so callers written against the reference
  (``c.actions()[:] = a; c.step(); c.observations()``) run unchanged.

There is no CPU fallback: if libmgx.so (the HIP build) is missing this module raises at first use.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from .compiler import Program, compile_spec
from .fmt import K
from .signature import objects_from_raw, stats_dicts

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MGX_LIB") or os.path.join(_HERE, "libmgx.so")  # MGX_LIB: instrumented dev builds
_lib = None
OBJ_RECORD_WORDS = 42

ENV_TOKEN_OVERFLOW, ENV_INVALID_KEY_RANGE, ENV_DEPTH, ENV_TOO_MANY_OBJECTS, ENV_TOKEN_POOL = 1, 2, 4, 8, 16
ENV_PROXY_INVENTORY, ENV_AGENT_LIFECYCLE = 32, 64   # territory proxy given an inventory / an agent spawned or removed
ENV_BAD_STATE = 128   # load_envs / copy_envs: a record of another layout; the env was left untouched


class MgxError(RuntimeError):
    pass


class EnvStateInfo(C.Structure):
    """include/mgx.h mgx_env_state_info: what decides whether a saved env state can be loaded."""
    _fields_ = [("record_bytes", C.c_int64), ("format", C.c_uint64), ("version", C.c_int32), ("pool_tokens", C.c_int32),
                ("n_segments", C.c_int32), ("reserved", C.c_int32)]

    def to_dict(self) -> dict:
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


def env_state_layout(prog: Program, class_maps) -> dict:
    """The env-state info an engine created from ``prog`` and ``class_maps`` [n, H, W] would report (host-only)."""
    cm = np.ascontiguousarray(class_maps, dtype=np.uint16)
    if cm.ndim == 2:
        cm = cm[None]
    words = np.ascontiguousarray(prog.words, dtype=np.int32)
    info = EnvStateInfo()
    _check(load_lib().mgx_env_state_layout(words.ctypes.data, words.size, cm.ctypes.data, cm.shape[0], C.byref(info)))
    return info.to_dict()


class EnvState:
    """Saved state of some envs (include/mgx.h mgx_save_envs): ``data`` uint8 [n, record_bytes] — a torch tensor on the
    engine's device, or numpy after ``.cpu()`` / ``from_dict`` —, the layout info it was saved with and ``envs``, the slots
    it was saved from.  ``to_dict()`` holds only numpy arrays and ints (``torch.save`` / ``np.savez``)."""

    INFO = ("record_bytes", "format", "version", "pool_tokens", "n_segments", "reserved")

    def __init__(self, data, info: dict, envs, extra: dict | None = None) -> None:
        self.data = data
        self.info = {k: int(info[k]) for k in self.INFO}
        self.envs = np.asarray(envs, dtype=np.int64).reshape(-1)
        self.extra = dict(extra or {})   # host-side companions (MettaGridBatchedEnv: episode counters)
        if tuple(data.shape) != (len(self.envs), self.info["record_bytes"]):
            raise ValueError(f"state data has shape {tuple(data.shape)}, expected {(len(self.envs), self.info['record_bytes'])}")

    def __len__(self) -> int:
        return len(self.envs)

    def cpu(self) -> "EnvState":
        d = self.data
        return EnvState(d if isinstance(d, np.ndarray) else d.cpu().numpy(), self.info, self.envs, self.extra)

    def to(self, device) -> "EnvState":
        import torch
        d = torch.as_tensor(self.data) if isinstance(self.data, np.ndarray) else self.data
        return EnvState(d.to(device).contiguous(), self.info, self.envs, self.extra)

    def to_dict(self) -> dict:
        out = {"data": np.ascontiguousarray(self.cpu().data), "envs": self.envs.copy()}
        out.update({f"info_{k}": np.array(v, dtype=np.uint64 if k == "format" else np.int64) for k, v in self.info.items()})
        out.update({f"extra_{k}": np.asarray(v) for k, v in self.extra.items()})
        return out

    @classmethod
    def from_dict(cls, d) -> "EnvState":
        info = {k: int(np.asarray(d[f"info_{k}"])) for k in cls.INFO}
        extra = {k[6:]: np.asarray(d[k]) for k in d.keys() if k.startswith("extra_")}
        return cls(np.ascontiguousarray(np.asarray(d["data"], dtype=np.uint8)), info, np.asarray(d["envs"]), extra)

    def info_struct(self) -> EnvStateInfo:
        return EnvStateInfo(**self.info)


def env_list(envs, E: int, what: str, unique: bool = False) -> np.ndarray:
    """``envs`` (None = all) as a contiguous int32 array of valid env indices, else ValueError."""
    if envs is None:
        return np.arange(E, dtype=np.int32)
    a = np.asarray(envs)
    if a.ndim == 0:
        a = a.reshape(1)
    if a.ndim != 1 or a.size == 0:
        raise ValueError(f"{what}: needs a non-empty 1-d list of env indices")
    if a.dtype.kind not in "iu":
        raise ValueError(f"{what}: env indices must be integers, not {a.dtype}")
    if a.min() < 0 or a.max() >= E:
        raise ValueError(f"{what}: env index out of range [0, {E}): {a.tolist()}")
    if unique and len(np.unique(a)) != a.size:
        raise ValueError(f"{what}: a destination env is listed twice: {a.tolist()}")
    return np.ascontiguousarray(a, dtype=np.int32)


def load_lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise MgxError(
            f"{LIB_PATH} not found: the HIP engine is not built. Run `python -c 'import __graft_entry__ as g; "
            "g.build()'` (hipcc --offload-arch=gfx950). There is no CPU fallback.")
    try:  # one HIP runtime per process: torch bundles libamdhip64.so.7; load it first so libmgx binds to the same one
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(LIB_PATH)
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    L.mgx_last_error.restype = C.c_char_p
    L.mgx_create.argtypes = [vp, C.c_size_t, vp, vp, i32, i32, C.POINTER(vp)]
    L.mgx_destroy.argtypes = [vp]
    L.mgx_destroy.restype = None
    L.mgx_set_buffers.argtypes = [vp, vp, vp, vp, vp, vp, vp, i64, i64, i32]
    L.mgx_step.argtypes = [vp]
    L.mgx_reset_envs.argtypes = [vp, vp, vp, vp]
    L.mgx_sync.argtypes = [vp]
    L.mgx_stream.argtypes = [vp]
    L.mgx_stream.restype = vp
    L.mgx_chain_world.argtypes = [vp, vp]
    L.mgx_wait_before_outputs.argtypes = [vp, vp]
    L.mgx_set_joint_actions.argtypes = [vp, vp, i32, vp, i32]
    L.mgx_poll_action_errors.argtypes = [vp, i32, C.POINTER(C.c_uint32), C.POINTER(i64), C.POINTER(i32)]
    L.mgx_get_buffers.argtypes = [vp] + [C.POINTER(vp)] * 6 + [C.POINTER(i32)]
    L.mgx_get_episode_rewards.argtypes = [vp, vp]
    L.mgx_get_action_success.argtypes = [vp, vp]
    L.mgx_get_current_steps.argtypes = [vp, vp]
    L.mgx_get_executed_actions.argtypes = [vp, vp]
    L.mgx_invalidate_observations.argtypes = [vp]
    L.mgx_get_observation_counts.argtypes = [vp, vp]
    L.mgx_get_stats.argtypes = [vp, i32, vp, vp, vp, vp]
    L.mgx_get_objects.argtypes = [vp, i32, vp, C.POINTER(i32)]
    L.mgx_get_objects_batch.argtypes = [vp, vp, i32, vp, vp]
    L.mgx_get_invalid_index_extra.argtypes = [vp, i32, vp, vp]
    L.mgx_get_reward_state.argtypes = [vp, i32, vp]
    L.mgx_poll_errors.argtypes = [vp, C.POINTER(C.c_uint32), C.POINTER(i32)]
    L.mgx_set_inventory.argtypes = [vp, i32, i32, vp, vp, i32]
    L.mgx_decode_obs.argtypes = [vp, vp, i64, vp, i32, vp]
    L.mgx_set_box_output.argtypes = [vp, vp, i32, i32, vp]
    L.mgx_token_bag.argtypes = [vp, vp, i64, vp, i32, vp, i32, vp]
    L.mgx_render_cells.argtypes = [vp, vp, i32, vp]
    L.mgx_set_render_tiles.argtypes = [vp, vp, i32, i32, vp, vp, vp, i32]
    L.mgx_render_rgb.argtypes = [vp, vp, i32, vp]
    L.mgx_state_digests.argtypes = [vp, vp]
    L.mgx_set_map_pool.argtypes = [vp, vp, i32]
    L.mgx_reset_envs_from_pool.argtypes = [vp, vp, vp, vp]
    L.mgx_set_auto_reset.argtypes = [vp, i32, i32, vp]
    L.mgx_get_episodes.argtypes = [vp, vp, vp]
    L.mgx_set_episode_stats.argtypes = [vp, i32, i32, i32]
    L.mgx_episode_stats_layout.argtypes = [vp, vp]
    L.mgx_record_episodes.argtypes = [vp, vp]
    L.mgx_request_episode_stats.argtypes = [vp]
    L.mgx_fetch_episode_stats.argtypes = [vp, i32, vp, C.POINTER(i32)]
    L.mgx_drain_episode_log.argtypes = [vp, vp, i32, C.POINTER(i32), C.POINTER(i32)]
    L.mgx_set_time_averages.argtypes = [vp, i32, i32]
    L.mgx_time_average_layout.argtypes = [vp, vp]
    L.mgx_time_average_layout_of.argtypes = [i32, i32, vp]
    L.mgx_request_time_averages.argtypes = [vp]
    L.mgx_fetch_time_averages.argtypes = [vp, i32, vp, C.POINTER(i32)]
    L.mgx_drain_time_average_log.argtypes = [vp, vp, i32, C.POINTER(i32), C.POINTER(i32)]
    L.mgx_get_time_average_state.argtypes = [vp, vp, i32, vp, vp, vp]
    L.mgx_put_time_average_state.argtypes = [vp, vp, i32, vp, vp, vp]
    L.mgx_set_policy_stats.argtypes = [vp, i32, i32, vp, i32]
    L.mgx_set_policy_assignments.argtypes = [vp, vp, i32, vp]
    L.mgx_policy_stats_layout.argtypes = [vp, vp]
    L.mgx_policy_stats_layout_of.argtypes = [i32, i32, i32, i32, vp]
    L.mgx_request_policy_stats.argtypes = [vp]
    L.mgx_fetch_policy_stats.argtypes = [vp, i32, vp, C.POINTER(i32)]
    L.mgx_drain_policy_log.argtypes = [vp, vp, i32, C.POINTER(i32), C.POINTER(i32)]
    L.mgx_count_objects_with_tag.argtypes = [vp, i32, i32, C.POINTER(i32)]
    L.mgx_set_profiling.argtypes = [vp, i32]
    L.mgx_get_step_timing.argtypes = [vp, vp]
    L.mgx_attach_code.argtypes = [vp, i32, C.c_char_p]
    if hasattr(L, "mgx_pack_rows"):   # (absent from the CPU sanitizer build, tests/cpu_emu: wavefront-cooperative kernels)
        L.mgx_pack_scratch_bytes.argtypes = [i64]
        L.mgx_pack_scratch_bytes.restype = i64
        L.mgx_pack_rows.argtypes = [vp, i64, i32, vp, vp, i64, vp, vp]
        L.mgx_pack_result.argtypes = [vp, i64, C.POINTER(i64), C.POINTER(i32), vp]
        L.mgx_unpack_rows.argtypes = [vp, vp, i64, i32, vp, vp, vp]
    if hasattr(L, "mgx_byte_linear_forward"):   # (absent from the CPU sanitizer build: no MFMA stand-in)
        L.mgx_byte_linear_forward.argtypes = [vp, i64, i32, i64, vp, vp, i32, vp, C.c_float, vp, i32, i64, i32, vp]
        L.mgx_byte_linear_wgrad.argtypes = [vp, i64, i32, i64, vp, i32, i32, i32, C.c_float, vp, vp, vp]
        L.mgx_byte_linear_scratch_bytes.argtypes = [i64, i32, i32]
        L.mgx_byte_linear_scratch_bytes.restype = i64
        L.mgx_byte_linear_chunk_rows.argtypes = []
        L.mgx_byte_linear_chunk_rows.restype = i32
    if hasattr(L, "mgx_sample_actions"):        # (absent from the CPU sanitizer build: wavefront-cooperative kernels)
        u64 = C.c_uint64
        L.mgx_sample_actions.argtypes = [vp, i32, i64, i32, i64, vp, C.c_float, i32, u64, u64, vp, vp, vp, vp, vp]
        L.mgx_action_logprob.argtypes = [vp, i32, i64, i32, i64, vp, C.c_float, vp, vp, vp, vp, vp]
        L.mgx_action_logprob_backward.argtypes = [vp, i32, i64, i32, i64, vp, C.c_float, vp, vp, vp, vp, i32, i64, vp]
    for name in ("mgx_num_envs", "mgx_num_agents", "mgx_num_tokens", "mgx_obs_variant", "mgx_act_variant", "mgx_handler_variant",
                 "mgx_world_prog_in_lds", "mgx_is_extended", "mgx_dispatch_pairs", "mgx_integer_bookkeeping",
                 "mgx_create_paths", "mgx_move_fast", "mgx_world_variant"):
        getattr(L, name).argtypes = [vp]
        getattr(L, name).restype = i32
    L.mgx_move_fast_counts.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.mgx_world_shape_fields.argtypes = [vp, C.c_size_t, vp, i32]
    L.mgx_world_shape_fields.restype = i32
    L.mgx_state_bytes.argtypes = [vp]
    L.mgx_state_bytes.restype = i64
    L.mgx_env_state_layout.argtypes = [vp, C.c_size_t, vp, i32, C.POINTER(EnvStateInfo)]
    L.mgx_env_state_info.argtypes = [vp, C.POINTER(EnvStateInfo)]
    L.mgx_save_envs.argtypes = [vp, vp, i32, vp]
    L.mgx_load_envs.argtypes = [vp, vp, i32, vp, C.POINTER(EnvStateInfo)]
    L.mgx_copy_envs.argtypes = [vp, vp, vp, i32]
    L.mgx_set_replay.argtypes = [vp, vp, i32, i32, vp, i32]
    L.mgx_replay_layout.argtypes = [vp, vp]
    L.mgx_drain_replay.argtypes = [vp, vp, vp, vp]
    if hasattr(L, "mgx_set_step_stats"):      # (absent from the CPU sanitizer build)
        L.mgx_set_step_stats.argtypes = [vp, vp, i32, vp, i32, vp, vp, vp, vp]
        L.mgx_step_stats_columns.argtypes = [vp, vp]
    if hasattr(L, "mgx_set_global_state"):    # (absent from the CPU sanitizer build)
        L.mgx_global_state_bound.argtypes = [vp, vp, C.POINTER(i32)]
        L.mgx_set_global_state.argtypes = [vp, vp, i32, vp, vp, vp]
        L.mgx_write_global_state.argtypes = [vp, vp]
    if hasattr(L, "mgx_set_map_generator"):   # (absent from the CPU sanitizer build, like the packed rows)
        L.mgx_set_map_generator.argtypes = [vp, vp, i32, i32, i32, vp, vp, i32, vp]
        L.mgx_set_map_scene_generator.argtypes = [vp] + [i32] * 10 + [vp, i32, vp, vp, i32, vp]
        L.mgx_set_map_maze_generator.argtypes = [vp] + [i32] * 15 + [vp, i32, vp, vp, i32, vp]
        L.mgx_generate_maps.argtypes = [vp, vp, i32, vp, i32]
        L.mgx_reset_envs_generated.argtypes = [vp, vp, vp, vp]
        L.mgx_get_map_seeds.argtypes = [vp, vp]
    if hasattr(L, "mgx_set_pool_sampling"):   # (absent from the CPU sanitizer build)
        u32 = C.c_uint32
        L.mgx_pool_quantise.argtypes = [vp, i32, vp]
        L.mgx_pool_draw_words.argtypes = [u32, vp, vp, i32, vp]
        L.mgx_set_pool_sampling.argtypes = [vp, vp, u32, u32]
        L.mgx_set_pool_weights.argtypes = [vp, vp]
        L.mgx_pool_draws.argtypes = [vp, vp, vp, i32, vp]
        L.mgx_set_map_stats.argtypes = [vp, i32]
        L.mgx_request_map_stats.argtypes = [vp]
        L.mgx_fetch_map_stats.argtypes = [vp, i32, vp, C.POINTER(i32)]
    _lib = L
    return L


# bit i of mgx_create_paths (include/mgx.h MGX_PATH_*, in bit order)
PATH_BITS = ("X", "prog_lds", "aoe_local", "tick_in_aoe", "cov_in_aoe", "aoe_prog_lds", "x_aoe_lds", "flat_top", "tick_split",
             "act_par", "duo", "act_map", "shadow", "rewards_early", "rewards_mid", "rewards_ext", "obs_512", "world_lds_64k",
             "gen")


def exported_symbols() -> list:
    """Entry points declared in include/mgx.h (used by the CPU-side ABI test)."""
    import re
    hdr = open(os.path.join(os.path.dirname(_HERE), "include", "mgx.h")).read()
    hdr = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    return sorted(set(re.findall(r"\b(mgx_[a-z_]+)\s*\(", hdr)))


def _check(rc: int) -> None:
    if rc != 0:
        msg = load_lib().mgx_last_error().decode()
        if rc == -1:
            raise ValueError(msg) if "shape" not in msg and "token" not in msg else RuntimeError(msg)
        raise MgxError(f"libmgx error {rc}: {msg}")


class BatchedMettaGrid:
    """E independent envs stepped together on one MI355X.

    ``buffers="device"``: observation/reward/terminal/truncation/action buffers are torch CUDA tensors owned by this
    object (or passed in through ``set_buffers``) and the kernels write into them directly.
    ``buffers="host"``: numpy arrays; actions are uploaded and results downloaded on every step (PCIe-inclusive).
    """

    def __init__(self, prog: Program, class_maps: np.ndarray, seeds, device: int = 0, buffers: str = "device",
                 specialize="auto") -> None:
        """``specialize``: compile the world / observation kernels for THIS program in the background and switch to them when
        they are ready (mettagrid_amd/jit.py; results are identical).  ``"auto"``: for batches of at least 1 024 envs whose
        program is not one the build already specialised; ``"async"`` / ``"sync"`` (wait in the constructor): always;
        ``False``: never."""
        self.L = load_lib()
        self.prog = prog
        cm = np.ascontiguousarray(class_maps, dtype=np.uint16)
        H, W = int(prog.words[K.H_HEIGHT]), int(prog.words[K.H_WIDTH])
        if cm.ndim == 2:
            cm = cm[None]
        if cm.shape[1:] != (H, W):
            raise ValueError(f"class_maps has shape {cm.shape} but the program was compiled for {H}x{W} maps")
        self.E = cm.shape[0]
        self.A, self.T = prog.num_agents, prog.num_tokens
        seeds = np.ascontiguousarray(np.broadcast_to(np.asarray(seeds, dtype=np.uint32), (self.E,)))
        words = np.ascontiguousarray(prog.words, dtype=np.int32)
        self.device = device
        self.h = C.c_void_p()
        _check(self.L.mgx_create(words.ctypes.data, words.size, cm.ctypes.data, seeds.ctypes.data, self.E, device,
                                 C.byref(self.h)))
        self.kind = buffers
        rows = self.E * self.A
        if isinstance(buffers, dict):   # the caller's own device tensors (e.g. slices of one batch: EnvGroups)
            self.kind = "device"
            want = {"obs": ((rows, self.T, 3), "uint8"), "terminals": ((rows,), "bool"), "truncations": ((rows,), "bool"),
                    "rewards": ((rows,), "float32"), "actions": ((rows,), "int32"), "vibe_actions": ((rows,), "int32")}
            for name, (shape, dt) in want.items():
                t = buffers[name]
                if tuple(t.shape) != shape or str(t.dtype) != "torch." + dt or not t.is_contiguous() or t.device.index != device:
                    raise ValueError(f"buffer {name!r} must be a contiguous {dt}{list(shape)} tensor on cuda:{device}")
                setattr(self, name, t)
            self._bind(*(t.data_ptr() for t in (self.obs, self.terminals, self.truncations, self.rewards,
                                                self.actions, self.vibe_actions)), mem_kind=1)
        elif buffers == "device":
            import torch
            dev = torch.device("cuda", device)
            self.obs = torch.empty((rows, self.T, 3), dtype=torch.uint8, device=dev)
            self.terminals = torch.empty(rows, dtype=torch.bool, device=dev)
            self.truncations = torch.empty(rows, dtype=torch.bool, device=dev)
            self.rewards = torch.empty(rows, dtype=torch.float32, device=dev)
            self.actions = torch.zeros(rows, dtype=torch.int32, device=dev)
            self.vibe_actions = torch.zeros(rows, dtype=torch.int32, device=dev)
            torch.cuda.synchronize(dev)
            self._bind(*(t.data_ptr() for t in (self.obs, self.terminals, self.truncations, self.rewards,
                                                self.actions, self.vibe_actions)), mem_kind=1)
        elif buffers == "host":
            self.obs = np.empty((rows, self.T, 3), np.uint8)
            self.terminals = np.zeros(rows, np.bool_)
            self.truncations = np.zeros(rows, np.bool_)
            self.rewards = np.zeros(rows, np.float32)
            self.actions = np.zeros(rows, np.int32)
            self.vibe_actions = np.zeros(rows, np.int32)
            self._bind(*(a.ctypes.data for a in (self.obs, self.terminals, self.truncations, self.rewards,
                                                 self.actions, self.vibe_actions)), mem_kind=0)
        else:
            raise ValueError("buffers must be 'device' or 'host'")
        self._jit_jobs, self.jit_errors = [], []
        if specialize and (specialize != "auto" or self.E >= 1024):
            self._start_jit(wait=specialize == "sync")

    # ---- run-time specialisation (include/mgx.h mgx_attach_code) ----
    def _start_jit(self, wait: bool = False) -> None:
        from . import jit
        if not jit.enabled():
            return
        if self.L.mgx_is_extended(self.h):   # extended programs: the lane-per-agent dispatch kernel, when the engine runs it
            kinds = ["actx"] if self.act_variant == 1 and self.handler_variant == 0 and self.L.mgx_world_prog_in_lds(self.h) else []
        else:
            kinds = [k for k, have in (("world", self.handler_variant != 0 or self.act_variant != 0), ("obs", self.obs_variant != 0)) if not have]
        if kinds:
            self._jit_jobs = jit.start(self.prog, bool(self.L.mgx_world_prog_in_lds(self.h)), kinds)
        if wait:
            for j in self._jit_jobs:
                j.wait()
        self._poll_jit()

    def _poll_jit(self) -> None:
        from . import jit
        for j in list(self._jit_jobs):
            if not j.ready():
                continue
            self._jit_jobs.remove(j)
            if j.error is None:
                rc = self.L.mgx_attach_code(self.h, jit.KINDS[j.kind], j.path.encode())
                if rc != 0:
                    j.error = self.L.mgx_last_error().decode()
            if j.error is not None:   # the generic kernels stay: slower, same results
                self.jit_errors.append((j.kind, j.error))
                if os.environ.get("MGX_VERBOSE"):
                    print(f"[mgx] run-time specialisation of the {j.kind} kernel failed: {j.error}", flush=True)

    def jit_pending(self) -> bool:
        """True while a code object for this engine is still compiling (``step`` attaches it when it is done)."""
        return bool(self._jit_jobs)

    def _bind(self, obs, term, trunc, rew, act, vact, mem_kind: int, rows=None, tokens=None) -> None:
        _check(self.L.mgx_set_buffers(self.h, obs, term, trunc, rew, act, vact,
                                      self.E * self.A if rows is None else rows,
                                      self.T if tokens is None else tokens, mem_kind))

    def close(self) -> None:
        if getattr(self, "h", None) and self.h:
            self.L.mgx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- stepping ----
    def step(self, check_errors: bool = False) -> None:
        if self._jit_jobs:
            self._poll_jit()
        _check(self.L.mgx_step(self.h))
        if check_errors:
            self.raise_env_errors()

    def sync(self) -> None:
        _check(self.L.mgx_sync(self.h))

    def set_joint_actions(self, joint, num_primary: int, vibe_ids) -> None:
        """One joint discrete id per agent -> the engine's primary / vibe action buffers, decoded on the device on the
        engine's stream (mgx.h mgx_set_joint_actions; MettaGridPufferEnv.step's decoding without its range checks).
        ``joint``: contiguous int32 CUDA tensor [E*A]; call ``wait_for_caller()`` first if it was written on another stream."""
        ids = np.ascontiguousarray(np.asarray(vibe_ids, dtype=np.int32))
        _check(self.L.mgx_set_joint_actions(self.h, joint.data_ptr(), int(num_primary), ids.ctypes.data if ids.size else None, int(ids.size)))

    def poll_action_errors(self, wait: bool = False):
        """(flags, row, value) of the range check ``set_joint_actions`` makes on the device (include/mgx.h
        mgx_poll_action_errors): flags 0 = all ids seen so far were in range.  ``wait=False`` does not synchronise."""
        flags, row, value = C.c_uint32(0), C.c_int64(-1), C.c_int32(0)
        _check(self.L.mgx_poll_action_errors(self.h, 1 if wait else 0, C.byref(flags), C.byref(row), C.byref(value)))
        return flags.value, row.value, value.value

    def chain_world_after(self, other: "BatchedMettaGrid | None") -> None:
        """From now on this engine's world-update kernels start only when ``other``'s most recent ones have finished
        (include/mgx.h mgx_chain_world): the building block of ``EnvGroups``."""
        _check(self.L.mgx_chain_world(self.h, other.h if other is not None else None))

    def wait_before_outputs(self, event) -> None:
        """The next engine work that writes observations / rewards / terminals / truncations waits for ``event`` (a recorded
        ``torch.cuda.Event``, kept alive here until then); the next step's world update does not (include/mgx.h
        mgx_wait_before_outputs).  Used by ``dist.GatherToRoot`` to order a step behind the staging copy of the previous one."""
        self._out_fences = (getattr(self, "_out_fences", []) + [event])[-4:]   # (several consumers: none is freed while pending)
        _check(self.L.mgx_wait_before_outputs(self.h, C.c_void_p(event.cuda_event)))

    def _per_env(self, a, dtype=np.uint8) -> np.ndarray:
        """An env mask (or another array with one entry per env) -> contiguous ``dtype`` [E]."""
        return np.ascontiguousarray(np.asarray(a, dtype=dtype).reshape(self.E))

    def _per_env_or_all(self, v, dtype):
        """One value for all envs, or one per env -> contiguous ``dtype`` [E]; None stays None."""
        return None if v is None else np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=dtype), (self.E,)))

    def reset_envs(self, env_mask, class_maps=None, seeds=None) -> None:
        """Restart the selected envs in place on the device (new episode): optional new maps / seeds for them.
        Their buffer rows are cleared and receive the initial observations, exactly like a fresh reference
        ``MettaGrid`` + ``set_buffers``."""
        mask, sd = self._per_env(env_mask), self._per_env_or_all(seeds, np.uint32)
        cm_ptr = None
        if class_maps is not None:
            cm = np.ascontiguousarray(class_maps, dtype=np.uint16)
            H, W = int(self.prog.words[K.H_HEIGHT]), int(self.prog.words[K.H_WIDTH])
            if cm.shape != (self.E, H, W):
                raise ValueError(f"class_maps must have shape {(self.E, H, W)} (only masked envs are read)")
            cm_ptr = cm.ctypes.data
        _check(self.L.mgx_reset_envs(self.h, mask.ctypes.data, cm_ptr, None if sd is None else sd.ctypes.data))

    # ---- device-resident map pool + auto-reset ----
    def set_map_pool(self, class_maps) -> None:
        """Upload finished maps once (uint16 [M, H, W], class index + 1); episodes then restart from them on the device."""
        cm = np.ascontiguousarray(class_maps, dtype=np.uint16)
        H, W = int(self.prog.words[K.H_HEIGHT]), int(self.prog.words[K.H_WIDTH])
        if cm.ndim != 3 or cm.shape[1:] != (H, W):
            raise ValueError(f"map pool must have shape [M, {H}, {W}]")
        _check(self.L.mgx_set_map_pool(self.h, cm.ctypes.data, cm.shape[0]))
        self.pool_size = cm.shape[0]

    def reset_envs_from_pool(self, env_mask, pool_index, seeds=None) -> None:
        mask, sd = self._per_env(env_mask), self._per_env_or_all(seeds, np.uint32)
        idx = self._per_env_or_all(np.asarray(pool_index), np.int32)
        _check(self.L.mgx_reset_envs_from_pool(self.h, mask.ctypes.data, idx.ctypes.data, None if sd is None else sd.ctypes.data))

    def set_auto_reset(self, enabled: bool = True, pool_stride: int = 1, early_end_steps=None) -> None:
        """Lazy auto-reset on the device (MettaGridPufferEnv.step, mettagrid_puffer_env.py:299-302); ``early_end_steps``
        [E]: step at which each env's first episode is truncated early (EarlyResetHandler), 0 = never."""
        ee = None if early_end_steps is None else self._per_env(early_end_steps, np.uint32)
        _check(self.L.mgx_set_auto_reset(self.h, 1 if enabled else 0, int(pool_stride), None if ee is None else ee.ctypes.data))

    def episodes(self):
        ep, mi = np.empty(self.E, np.uint32), np.empty(self.E, np.int32)
        _check(self.L.mgx_get_episodes(self.h, ep.ctypes.data, mi.ctypes.data))
        return ep, mi

    # ---- device map generator (include/mgx.h "Device map generator"; csrc/mgx_mapgen.h) ----
    def set_map_generator(self, spec, map_seed_base=0) -> None:
        """New episodes' maps from one of the reference's map builders on the device.  ``spec``: a ``mapgen.RandomMapSpec``
        (RandomMapBuilder), a ``mapgen.MapGenSpec`` (MapGen with a Random instance scene, the arena's builder) or a
        ``mapgen.MazeGenSpec`` (MapGen with a Maze instance scene and a Random child), or what their ``lower(prog)`` returns; the
        engine holds one recipe, so setting one replaces the other and ``None`` switches the
        generator off; ``map_seed_base``: uint32 [E] (or one value for all)."""
        if spec is None:
            _check(self.L.mgx_set_map_generator(self.h, None, 0, 0, 0, None, None, 0, None))
            return
        low = spec.lower(self.prog) if hasattr(spec, "lower") else spec
        rename = np.ascontiguousarray(low.rename, dtype=np.uint16)
        off = np.ascontiguousarray(low.rename_off, dtype=np.int32)
        base = np.ascontiguousarray(np.broadcast_to(np.asarray(map_seed_base, dtype=np.uint32), (self.E,)))
        n_teams = int(off.size) - 1
        tables = (rename.ctypes.data if rename.size else None, off.ctypes.data if n_teams > 0 else None, n_teams, base.ctypes.data)
        if not hasattr(low, "symbols"):   # a mapgen.LoweredMap
            inner = np.ascontiguousarray(low.inner, dtype=np.uint16)
            _check(self.L.mgx_set_map_generator(self.h, inner.ctypes.data, int(inner.size), int(low.border_width), int(low.border_code), *tables))
            return
        sym = np.ascontiguousarray(low.symbols, dtype=np.uint16)
        rooms = [int(v) for v in (low.room_height, low.room_width, low.n_inst, low.rows, low.cols, low.border_width, low.instance_border_width,
                                  low.border_code, low.instance_border_code)]
        tail = (sym.ctypes.data if sym.size else None, int(low.n_sym), *tables)
        if hasattr(low, "algorithm"):   # a mapgen.LoweredMaze
            _check(self.L.mgx_set_map_maze_generator(self.h, *rooms, int(low.algorithm), int(low.room_size), int(low.wall_size), int(low.wall_code),
                                                     int(bool(low.first_on_root)), int(low.key_offset), *tail))
        else:                           # a mapgen.LoweredScene
            _check(self.L.mgx_set_map_scene_generator(self.h, *rooms, int(bool(low.first_on_root)), *tail))

    def generate_maps(self, map_seeds, out=None):
        """The generator's maps for ``map_seeds`` (uint32 [n]) -> uint16 [n, H, W]; no env is touched.  ``out``: a contiguous
        torch int16 / uint16 device tensor of that shape to fill instead of returning a numpy array; the engine's stream
        waits for what the caller's current torch stream has enqueued (whatever produced ``out``) before it writes, and the
        call returns once the maps have landed."""
        sd = np.ascontiguousarray(np.asarray(map_seeds, dtype=np.uint32).reshape(-1))
        H, W = int(self.prog.words[K.H_HEIGHT]), int(self.prog.words[K.H_WIDTH])
        if out is not None:
            if tuple(out.shape) != (sd.size, H, W) or out.element_size() != 2 or not out.is_contiguous() or not out.is_cuda:
                raise ValueError(f"out must be a contiguous 16-bit device tensor of shape {(sd.size, H, W)}")
            self.wait_for_caller()
            _check(self.L.mgx_generate_maps(self.h, sd.ctypes.data, int(sd.size), C.c_void_p(out.data_ptr()), 1))
            return out
        maps = np.empty((sd.size, H, W), np.uint16)
        _check(self.L.mgx_generate_maps(self.h, sd.ctypes.data, int(sd.size), maps.ctypes.data, 0))
        return maps

    def reset_envs_generated(self, env_mask, map_seeds=None, seeds=None) -> None:
        """``reset_envs`` with the masked envs' maps generated on the device: ``map_seeds`` uint32 [E] (only masked envs are
        read) or None = each slot's base seed + its episode count."""
        mask = self._per_env(env_mask)
        ms, sd = self._per_env_or_all(map_seeds, np.uint32), self._per_env_or_all(seeds, np.uint32)
        _check(self.L.mgx_reset_envs_generated(self.h, mask.ctypes.data, None if ms is None else ms.ctypes.data,
                                               None if sd is None else sd.ctypes.data))

    def map_seeds(self) -> np.ndarray:
        """uint32 [E]: the seed of the map each env's most recent generated restart built."""
        out = np.empty(self.E, np.uint32)
        _check(self.L.mgx_get_map_seeds(self.h, out.ctypes.data))
        return out

    # ---- weighted pool sampling and per-map statistics (include/mgx.h "Weighted map-pool sampling"; pool_sampling.py) ----
    def _pool_weights(self, weights) -> np.ndarray:
        M = getattr(self, "pool_size", 0)
        if M <= 0:
            raise ValueError("no map pool (set_map_pool)")
        w = np.ascontiguousarray(weights, dtype=np.float64)
        if w.shape != (M,):
            raise ValueError(f"weights must have shape [{M}], one per pool map")
        return w

    def set_pool_sampling(self, weights, sample_seed: int = 0, env_offset: int = 0) -> None:
        """Auto-resets draw the next pool map with probability proportional to ``weights`` (f64 [M]; ``None``: the rotation rule
        again): episode ``k`` of slot ``e`` plays ``pool_sampling.draws(weights, sample_seed, env_offset, [e], [k])``.
        ``env_offset``: the slot's global env index minus its index here (engines that share one batch)."""
        if weights is None:
            _check(self.L.mgx_set_pool_sampling(self.h, None, 0, 0))
            return
        w = self._pool_weights(weights)
        _check(self.L.mgx_set_pool_sampling(self.h, w.ctypes.data, int(sample_seed) & 0xFFFFFFFF, int(env_offset) & 0xFFFFFFFF))

    def set_pool_weights(self, weights) -> None:
        """New weights from the next step's restarts on; does not wait for the device."""
        w = self._pool_weights(weights)
        _check(self.L.mgx_set_pool_weights(self.h, w.ctypes.data))

    def pool_draws(self, envs, episodes) -> np.ndarray:
        """int32 [n]: the pool map slot ``envs[i]`` plays as its episode ``episodes[i]``, computed by the device kernel."""
        ev = np.ascontiguousarray(np.asarray(envs, dtype=np.int32).reshape(-1))
        ep = np.ascontiguousarray(np.asarray(episodes, dtype=np.uint32).reshape(-1))
        if ev.size != ep.size:
            raise ValueError("envs and episodes must have the same length")
        out = np.empty(ev.size, np.int32)
        _check(self.L.mgx_pool_draws(self.h, ev.ctypes.data, ep.ctypes.data, int(ev.size), out.ctypes.data))
        return out

    # ---- the snapshot / drain protocol the statistics reducers share ----
    def _fetch_totals(self, fn, shape, dtype, wait: bool):
        """One ``mgx_fetch_*`` call: the snapshot requested last as an array, or None (nothing requested, or still in flight)."""
        out = np.zeros(shape, dtype)
        ready = C.c_int32(0)
        _check(fn(self.h, 1 if wait else 0, out.ctypes.data, C.byref(ready)))
        return out if ready.value else None

    @staticmethod
    def _drain_totals(request, fetch, lo=None, hi=None):
        """Everything recorded up to now, synchronously: a snapshot still in flight (requested earlier, not fetched) is merged
        with a fresh one — sums and counts add, the entries indexed by ``lo`` take the minimum, those by ``hi`` the maximum."""
        first = fetch(True)                    # None unless a request was pending
        request()
        tot = fetch(True)
        if first is None:
            return tot
        merged = first + tot
        if lo is not None:
            merged[lo] = np.minimum(first[lo], tot[lo])
        if hi is not None:
            merged[hi] = np.maximum(first[hi], tot[hi])
        return merged

    def _drain_log(self, fn, cap: int, words: int, what: str) -> tuple:
        """One ``mgx_drain_*_log`` call: (uint32 [n][words] records, dropped count)."""
        if cap <= 0:
            raise ValueError(what)
        raw = np.zeros((cap, words), np.uint32)
        n, dropped = C.c_int32(0), C.c_int32(0)
        _check(fn(self.h, raw.ctypes.data, cap, C.byref(n), C.byref(dropped)))
        return raw[:n.value], dropped.value

    def set_map_stats(self, enabled: bool = True) -> None:
        """Per-map episode statistics reduced on the device (needs ``set_episode_stats`` and a pool)."""
        _check(self.L.mgx_set_map_stats(self.h, 1 if enabled else 0))
        self._ms_on = bool(enabled)

    def request_map_stats(self) -> None:
        _check(self.L.mgx_request_map_stats(self.h))

    def _fetch_ms_raw(self, wait: bool):
        return self._fetch_totals(self.L.mgx_fetch_map_stats, (self.pool_size + 1, 6), np.uint64, wait)

    def fetch_map_stats(self, wait: bool = False, raw: bool = False):
        """The snapshot requested last: one dict per pool map plus a last one for episodes without a pool index (a slot's first
        episode) — ``episodes``, ``terminated``, ``length_sum``, ``return_sum`` (= q_sum / 2**20), ``return_min``,
        ``return_max`` — or, with ``raw``, the uint64 [M + 1][6] table; None while its copy is still in flight."""
        from .pool_sampling import table_dicts
        t = self._fetch_ms_raw(wait)
        return None if t is None else t if raw else table_dicts(t)

    def drain_map_stats(self, raw: bool = False):
        """Everything recorded up to now, synchronously; a snapshot still in flight is merged with a fresh one."""
        from .pool_sampling import table_dicts
        with np.errstate(over="ignore"):       # (two's complement: the q sums add like the counts)
            t = self._drain_totals(self.request_map_stats, self._fetch_ms_raw, lo=(slice(None), 4), hi=(slice(None), 5))
        return t if raw else table_dicts(t)

    # ---- episode-end statistics (include/mgx.h "Episode-end statistics"; the reference's StatsTracker.on_episode_end) ----
    EPL = ("NG", "NS", "A", "TOTALS_WORDS", "REC_WORDS", "LOG_WORDS", "OFF_GAME", "OFF_GAME_BITS", "OFF_AGENT", "OFF_AGENT_BITS",
           "OFF_REWARDS", "OFF_PA", "OFF_PA_BITS", "OFF_INVK", "OFF_INVN", "PER_AGENT", "LOG_CAPACITY")
    EPT = ("episodes", "return_sum", "return_min", "return_max", "length_sum", "length_min", "length_max", "terminated")

    def set_episode_stats(self, enabled: bool = True, log_capacity: int = 0, log_per_agent: bool = False) -> None:
        """Reduce the stats of every finished env into batch totals on the device (and keep up to ``log_capacity`` per-episode
        records, with the per-agent rows if asked) before the auto-reset wipes them."""
        _check(self.L.mgx_set_episode_stats(self.h, 1 if enabled else 0, int(log_capacity), 1 if log_per_agent else 0))
        self._epl = None
        self._tal = None   # (the engine switches the time averages off with the statistics they ride on)
        self._psl = None   # (... and the per-policy statistics)
        self._ms_on = False  # (... and the per-map table)
        if enabled:
            out = np.zeros(len(self.EPL), np.int32)
            _check(self.L.mgx_episode_stats_layout(self.h, out.ctypes.data))
            self._epl = {k: int(v) for k, v in zip(self.EPL, out)}

    def record_episodes(self, env_mask) -> None:
        """Host-driven restarts: record the masked envs' episodes as finished now (call before ``reset_envs``)."""
        _check(self.L.mgx_record_episodes(self.h, self._per_env(env_mask).ctypes.data))

    def request_episode_stats(self) -> None:
        _check(self.L.mgx_request_episode_stats(self.h))

    def _fetch_raw(self, wait: bool):
        return self._fetch_totals(self.L.mgx_fetch_episode_stats, self._epl["TOTALS_WORDS"], np.float64, wait)

    def fetch_episode_stats(self, wait: bool = False):
        """The snapshot requested last as a dict (see ``episode_totals_dict``), or None while its copy is still in flight."""
        raw = self._fetch_raw(wait)
        return None if raw is None else self.episode_totals_dict(raw)

    def drain_episode_stats(self):
        """Everything recorded up to now, synchronously: a snapshot still in flight (requested earlier, not fetched) is merged
        with a fresh one (sums and counts add, minima / maxima combine)."""
        lo, hi = [2, 5], [3, 6]                # MGX_EPT_RETURN_MIN / LENGTH_MIN, ..._MAX
        return self.episode_totals_dict(self._drain_totals(self.request_episode_stats, self._fetch_raw, lo, hi))

    def episode_totals_dict(self, totals: np.ndarray) -> dict:
        """Raw totals -> {"episodes", "return_sum", ..., "game_sum": {name: f64}, "game_count": {name: int}, "agent_sum", "agent_count"}
        (only keys some finished episode held)."""
        NG, NS, H = self._epl["NG"], self._epl["NS"], len(self.EPT)
        out = {k: float(totals[i]) for i, k in enumerate(self.EPT)}
        out["episodes"] = int(out["episodes"])
        gs, gc = totals[H:H + NG], totals[H + NG:H + 2 * NG]
        as_, ac = totals[H + 2 * NG:H + 2 * NG + NS], totals[H + 2 * NG + NS:H + 2 * NG + 2 * NS]
        out["game_sum"] = {self.prog.game_stat_names[i]: float(gs[i]) for i in range(NG) if gc[i]}
        out["game_count"] = {self.prog.game_stat_names[i]: int(gc[i]) for i in range(NG) if gc[i]}
        out["agent_sum"] = {self.prog.agent_stat_names[i]: float(as_[i]) for i in range(NS) if ac[i]}
        out["agent_count"] = {self.prog.agent_stat_names[i]: int(ac[i]) for i in range(NS) if ac[i]}
        return out

    def drain_episode_log(self):
        """(list of per-episode dicts, dropped count).  Each dict: env, episode, map_index, seed, steps, flags, episode_rewards
        (f32 [A]), game {name: value}, agent {name: f64 mean over agents} — the reference's infos["game"] / infos["agent"] —
        and, with log_per_agent, per_agent [A] dicts (incl. the "action.invalid_index.<k>" keys without a stat column)."""
        Lw = self._epl
        raw, dropped = self._drain_log(self.L.mgx_drain_episode_log, Lw["LOG_CAPACITY"], Lw["LOG_WORDS"],
                                       "no episode log: set_episode_stats(log_capacity=...)")
        return [self.episode_record_dict(r) for r in raw], dropped

    def episode_record_dict(self, rec: np.ndarray) -> dict:
        Lw = self._epl
        NG, NS, A = Lw["NG"], Lw["NS"], Lw["A"]
        gnames, anames = self.prog.game_stat_names, self.prog.agent_stat_names

        def bits(off, n):
            w = rec[off:off + (n + 31) // 32]
            return [(int(w[i >> 5]) >> (i & 31)) & 1 for i in range(n)]
        gv = rec[Lw["OFF_GAME"]:Lw["OFF_GAME"] + NG].view(np.float32)
        gb = bits(Lw["OFF_GAME_BITS"], NG)
        av = np.ascontiguousarray(rec[Lw["OFF_AGENT"]:Lw["OFF_AGENT"] + 2 * NS]).view(np.float64)
        ab = bits(Lw["OFF_AGENT_BITS"], NS)
        out = {"env": int(rec[0]), "episode": int(rec[1]), "map_index": int(np.int32(rec[2])), "seed": int(rec[3]), "steps": int(rec[4]),
               "flags": int(rec[5]), "return_sum": float(np.ascontiguousarray(rec[6:8]).view(np.float64)[0]),
               "episode_rewards": rec[Lw["OFF_REWARDS"]:Lw["OFF_REWARDS"] + A].view(np.float32).copy(),
               "game": {gnames[i]: float(gv[i]) for i in range(NG) if gb[i]},
               "agent": {anames[i]: float(av[i]) for i in range(NS) if ab[i]}}
        if Lw["PER_AGENT"]:
            pa = rec[Lw["OFF_PA"]:Lw["OFF_PA"] + A * NS].view(np.float32).reshape(A, NS)
            nsw = (NS + 31) // 32
            ik = rec[Lw["OFF_INVK"]:Lw["OFF_INVK"] + A * K.INVALID_EXTRA].view(np.int32).reshape(A, K.INVALID_EXTRA)
            inn = rec[Lw["OFF_INVN"]:Lw["OFF_INVN"] + A * K.INVALID_EXTRA].view(np.float32).reshape(A, K.INVALID_EXTRA)
            per = []
            for a in range(A):
                pb = bits(Lw["OFF_PA_BITS"] + a * nsw, NS)
                dct = {anames[i]: float(pa[a, i]) for i in range(NS) if pb[i]}
                for q in range(K.INVALID_EXTRA):
                    if inn[a, q] != 0:
                        dct[f"action.invalid_index.{int(ik[a, q])}"] = float(inn[a, q])
                per.append(dct)
            out["per_agent"] = per
            extra = {}   # keys without a stat column take part in infos["agent"] like any other (stats_tracker.py:41-46)
            for dct in per:
                for k, v in dct.items():
                    if k.startswith("action.invalid_index.") and k not in anames:
                        extra[k] = extra.get(k, 0) + v
            for k, v in extra.items():
                out["agent"][k] = v / A
        return out

    # ---- time-averaged game stats (include/mgx.h "Time-averaged game stats"; the reference's TimeAveragedStatsHandler) ----
    TAL = ("NG", "SEEN_WORDS", "REC_WORDS", "LOG_WORDS", "HEADER_WORDS", "OFF_AVG", "OFF_SEEN", "TOTALS_WORDS", "TOTALS_HEADER",
           "LOG_CAPACITY")
    TA_PARTIAL = 2   # record flags, bit 1

    def set_time_averages(self, enabled: bool = True, log_capacity: int = 0) -> None:
        """Accumulate every env's game stats after every step on the device and finish ``sum / steps`` per key when its
        episode ends (time_averaged_stats.py:17-41).  Needs ``set_episode_stats``."""
        _check(self.L.mgx_set_time_averages(self.h, 1 if enabled else 0, int(log_capacity)))
        self._tal = None
        if enabled:
            out = np.zeros(len(self.TAL), np.int32)
            _check(self.L.mgx_time_average_layout(self.h, out.ctypes.data))
            self._tal = {k: int(v) for k, v in zip(self.TAL, out)}

    def _ta_layout(self) -> dict:
        if getattr(self, "_tal", None) is None:
            raise ValueError("time averages are off: set_time_averages()")
        return self._tal

    def time_average_state(self, envs) -> dict:
        """Raw accumulators of ``envs``: {"sum": f64 [n][NG], "steps": u32 [n], "seen": u32 [n][SEEN_WORDS]}.  Synchronises."""
        Lw = self._ta_layout()
        lst = env_list(envs, self.E, "time_average_state")
        out = {"sum": np.zeros((len(lst), Lw["NG"]), np.float64), "steps": np.zeros(len(lst), np.uint32),
               "seen": np.zeros((len(lst), Lw["SEEN_WORDS"]), np.uint32)}
        _check(self.L.mgx_get_time_average_state(self.h, lst.ctypes.data, len(lst), out["sum"].ctypes.data, out["steps"].ctypes.data,
                                                 out["seen"].ctypes.data))
        return out

    def put_time_average_state(self, envs, state: dict) -> None:
        """Write accumulators read by ``time_average_state`` into ``envs`` (e.g. behind ``load_envs``)."""
        Lw = self._ta_layout()
        lst = env_list(envs, self.E, "put_time_average_state", unique=True)
        sums = np.ascontiguousarray(state["sum"], dtype=np.float64)
        steps = np.ascontiguousarray(state["steps"], dtype=np.uint32)
        seen = np.ascontiguousarray(state["seen"], dtype=np.uint32)
        if sums.shape != (len(lst), Lw["NG"]) or steps.shape != (len(lst),) or seen.shape != (len(lst), Lw["SEEN_WORDS"]):
            raise ValueError(f"put_time_average_state: accumulators of shape {sums.shape}, {steps.shape}, {seen.shape} for "
                             f"{len(lst)} envs, {Lw['NG']} game stats")
        _check(self.L.mgx_put_time_average_state(self.h, lst.ctypes.data, len(lst), sums.ctypes.data, steps.ctypes.data, seen.ctypes.data))

    def _ta_keys(self, values, seen_words) -> dict:
        names = self.prog.game_stat_names
        return {names[i]: float(values[i]) for i in range(len(values)) if (int(seen_words[i >> 5]) >> (i & 31)) & 1}

    def time_averages(self, envs) -> list:
        """``TimeAveragedStatsHandler.time_averaged_game_stats`` of ``envs`` read mid-episode: one {key: sum / steps} dict per
        env, {} at zero steps.  Synchronises with the device."""
        st = self.time_average_state(envs)
        return [self._ta_keys(st["sum"][k] / float(st["steps"][k]), st["seen"][k]) if st["steps"][k] else {} for k in range(len(st["steps"]))]

    def request_time_averages(self) -> None:
        _check(self.L.mgx_request_time_averages(self.h))

    def _fetch_ta_raw(self, wait: bool):
        return self._fetch_totals(self.L.mgx_fetch_time_averages, self._ta_layout()["TOTALS_WORDS"], np.float64, wait)

    def fetch_time_averages(self, wait: bool = False):
        """The snapshot requested last as a dict (see ``time_average_totals_dict``), or None while its copy is in flight."""
        raw = self._fetch_ta_raw(wait)
        return None if raw is None else self.time_average_totals_dict(raw)

    def drain_time_averages(self) -> dict:
        """Everything finished up to now, synchronously; a snapshot still in flight is added to a fresh one."""
        return self.time_average_totals_dict(self._drain_totals(self.request_time_averages, self._fetch_ta_raw))

    def time_average_totals_dict(self, totals: np.ndarray) -> dict:
        """Raw totals -> {"episodes", "partial", "sum": {key: f64 sum of the per-episode averages}, "count": {key: episodes
        holding the key}} (only keys some finished episode held; partial episodes are in neither)."""
        Lw = self._ta_layout()
        NG, H = Lw["NG"], Lw["TOTALS_HEADER"]
        names = self.prog.game_stat_names
        s, c = totals[H:H + NG], totals[H + NG:H + 2 * NG]
        return {"episodes": int(totals[0]), "partial": int(totals[1]),
                "sum": {names[i]: float(s[i]) for i in range(NG) if c[i]},
                "count": {names[i]: int(c[i]) for i in range(NG) if c[i]}}

    def drain_time_average_log(self):
        """(list of per-episode dicts, dropped count).  Each dict: env, episode, steps (the env's step at the end), ta_steps
        (steps accumulated), partial, time_averaged_game_stats {key: f64}."""
        Lw = self._ta_layout()
        NG = Lw["NG"]
        raw, dropped = self._drain_log(self.L.mgx_drain_time_average_log, Lw["LOG_CAPACITY"], Lw["LOG_WORDS"],
                                       "no time-average log: set_time_averages(log_capacity=...)")
        out = []
        for r in raw:
            avg = np.ascontiguousarray(r[Lw["OFF_AVG"]:Lw["OFF_AVG"] + 2 * NG]).view(np.float64)
            out.append({"env": int(r[0]), "episode": int(r[1]), "steps": int(r[2]), "ta_steps": int(r[3]),
                        "partial": bool(int(r[4]) & self.TA_PARTIAL),
                        "time_averaged_game_stats": self._ta_keys(avg, r[Lw["OFF_SEEN"]:Lw["OFF_SEEN"] + Lw["SEEN_WORDS"]])})
        return out, dropped

    # ---- per-policy episode statistics (include/mgx.h "Per-policy episode statistics"; multi_episode/summary.py:38-130) ----
    PSL = ("NS", "A", "P", "SEEN_WORDS", "REC_WORDS", "LOG_WORDS", "HEADER_WORDS", "OFF_REWARD", "OFF_COUNT", "OFF_SUM", "OFF_BITS",
           "TOTALS_WORDS", "TOTALS_HEADER", "TOTALS_POLICY_WORDS", "TOTALS_OFF_SUM", "TOTALS_OFF_COUNT", "LOG_CAPACITY")
    MAX_POLICIES = 16   # MGX_MAX_POLICIES

    def _policy_rows(self, rows, n: int, what: str) -> np.ndarray:
        """Assignments as a contiguous u8 [n][A]: one row for all (``[A]``) or one per env."""
        a = np.asarray(rows)
        if a.ndim == 1:
            a = np.broadcast_to(a, (n, len(a)))
        if a.shape != (n, self.A) or a.size == 0:
            raise ValueError(f"{what}: assignments of shape {np.asarray(rows).shape} for {n} envs of {self.A} agents")
        if (a < 0).any() or (a > 255).any():
            raise ValueError(f"{what}: a policy index outside [0, 255]")
        return np.ascontiguousarray(a, dtype=np.uint8)

    def set_policy_stats(self, enabled: bool = True, num_policies: int = 0, assignments=None, log_capacity: int = 0) -> None:
        """Reduce every finished episode's agent stats and returns per policy on the device; ``assignments``: the policy index
        of every agent row, ``[A]`` or ``[E][A]``.  Needs ``set_episode_stats``.  A refused call leaves the earlier setting."""
        if not enabled:
            _check(self.L.mgx_set_policy_stats(self.h, 0, 0, None, 0))
            self._psl = None
            return
        rows = self._policy_rows(assignments, self.E, "set_policy_stats")
        _check(self.L.mgx_set_policy_stats(self.h, 1, int(num_policies), rows.ctypes.data, int(log_capacity)))
        out = np.zeros(len(self.PSL), np.int32)
        _check(self.L.mgx_policy_stats_layout(self.h, out.ctypes.data))
        self._psl = {k: int(v) for k, v in zip(self.PSL, out)}

    def _ps_layout(self) -> dict:
        if getattr(self, "_psl", None) is None:
            raise ValueError("policy statistics are off: set_policy_stats()")
        return self._psl

    def set_policy_assignments(self, envs, rows) -> None:
        """Replace the assignment rows of ``envs`` (``rows``: ``[A]`` or ``[n][A]``), behind the steps enqueued so far."""
        self._ps_layout()
        lst = env_list(envs, self.E, "set_policy_assignments", unique=True)
        r = self._policy_rows(rows, len(lst), "set_policy_assignments")
        _check(self.L.mgx_set_policy_assignments(self.h, lst.ctypes.data, len(lst), r.ctypes.data))

    def request_policy_stats(self) -> None:
        _check(self.L.mgx_request_policy_stats(self.h))

    def _fetch_ps_raw(self, wait: bool):
        return self._fetch_totals(self.L.mgx_fetch_policy_stats, self._ps_layout()["TOTALS_WORDS"], np.float64, wait)

    def fetch_policy_stats(self, wait: bool = False):
        """The snapshot requested last as a dict (see ``policy_totals_dict``), or None while its copy is in flight."""
        raw = self._fetch_ps_raw(wait)
        return None if raw is None else self.policy_totals_dict(raw)

    def drain_policy_stats(self) -> dict:
        """Everything finished up to now, synchronously; a snapshot still in flight is merged with a fresh one (sums and
        counts add, minima / maxima combine)."""
        Lw = self._ps_layout()
        base = Lw["TOTALS_HEADER"] + Lw["TOTALS_POLICY_WORDS"] * np.arange(Lw["P"])
        lo, hi = base + 3, base + 4            # MGX_PSP_AVG_REWARD_MIN / _MAX
        return self.policy_totals_dict(self._drain_totals(self.request_policy_stats, self._fetch_ps_raw, lo, hi))

    def policy_totals_dict(self, totals: np.ndarray) -> dict:
        """Raw totals -> {"episodes", "policies": [{"episodes", "agent_episodes", "avg_reward_sum", "avg_reward_min",
        "avg_reward_max", "agent_sum": {key: f64}, "agent_count": {key: episodes}}]} (only keys some agent of the policy held)."""
        Lw = self._ps_layout()
        NS, P, H, W = Lw["NS"], Lw["P"], Lw["TOTALS_HEADER"], Lw["TOTALS_POLICY_WORDS"]
        names = self.prog.agent_stat_names
        pols = []
        for p in range(P):
            h = totals[H + W * p:H + W * (p + 1)]
            s = totals[Lw["TOTALS_OFF_SUM"] + p * NS:Lw["TOTALS_OFF_SUM"] + (p + 1) * NS]
            c = totals[Lw["TOTALS_OFF_COUNT"] + p * NS:Lw["TOTALS_OFF_COUNT"] + (p + 1) * NS]
            pols.append({"episodes": int(h[0]), "agent_episodes": int(h[1]), "avg_reward_sum": float(h[2]), "avg_reward_min": float(h[3]),
                         "avg_reward_max": float(h[4]),
                         "agent_sum": {names[i]: float(s[i]) for i in range(NS) if c[i]},
                         "agent_count": {names[i]: int(c[i]) for i in range(NS) if c[i]}})
        return {"episodes": int(totals[0]), "policies": pols}

    def drain_policy_log(self):
        """(list of per-episode dicts, dropped count); see ``policy_record_dict``."""
        Lw = self._ps_layout()
        raw, dropped = self._drain_log(self.L.mgx_drain_policy_log, Lw["LOG_CAPACITY"], Lw["LOG_WORDS"],
                                       "no policy log: set_policy_stats(log_capacity=...)")
        return [self.policy_record_dict(r) for r in raw], dropped

    def policy_record_dict(self, rec: np.ndarray) -> dict:
        """One record -> env, episode, steps, flags, reward_sum (f64 [P]), agents (int [P]), avg_rewards ([P] float or None:
        the episode's row of per_episode_per_policy_avg_rewards), policies [P] of {key: f64 sum over the policy's agents}."""
        Lw = self._ps_layout()
        NS, P, SW = Lw["NS"], Lw["P"], Lw["SEEN_WORDS"]
        names = self.prog.agent_stat_names
        rew = np.ascontiguousarray(rec[Lw["OFF_REWARD"]:Lw["OFF_REWARD"] + 2 * P]).view(np.float64).copy()
        cnt = rec[Lw["OFF_COUNT"]:Lw["OFF_COUNT"] + P].astype(np.int64)
        sums = np.ascontiguousarray(rec[Lw["OFF_SUM"]:Lw["OFF_SUM"] + 2 * P * NS]).view(np.float64).reshape(P, NS)
        bits = rec[Lw["OFF_BITS"]:Lw["OFF_BITS"] + P * SW].reshape(P, SW)
        return {"env": int(rec[0]), "episode": int(rec[1]), "steps": int(rec[2]), "flags": int(rec[3]), "reward_sum": rew, "agents": cnt,
                "avg_rewards": [float(rew[p] / cnt[p]) if cnt[p] > 0 else None for p in range(P)],
                "policies": [{names[i]: float(sums[p, i]) for i in range(NS) if (int(bits[p, i >> 5]) >> (i & 31)) & 1} for p in range(P)]}

    # ---- replays of watched envs (include/mgx.h "Replays"; mettagrid_amd/replay.py) ----
    RPL = ("NUM_ENVS", "WORDS_PER_ENV", "STEP_WORDS", "END_WORDS", "SLOT_WORDS", "AMOUNT_WORDS", "GROUPS", "OBJECT_SLOTS", "MAX_STEP_WORDS")

    def set_replay(self, envs, words_per_env: int | None = None, static_types=("wall",)) -> None:
        """Record the listed envs' episodes on the device: from the next step on, a kernel behind every step appends what
        changed in their objects to a per-env log of ``words_per_env`` uint32 (default: room for four keyframes of a full env).
        Objects whose type name is in ``static_types`` are logged in keyframes only (the reference's list).  An empty list
        switches the recorder off."""
        idx = np.ascontiguousarray(np.asarray(envs if envs is not None else [], dtype=np.int64).reshape(-1))
        self.replay_envs = []
        if idx.size == 0:
            _check(self.L.mgx_set_replay(self.h, None, 0, 0, None, 0))
            return
        if idx.min() < -2**31 or idx.max() >= 2**31:
            raise ValueError(f"set_replay: env index out of range [0, {self.E})")
        idx = idx.astype(np.int32)
        tids = np.ascontiguousarray([i for i, n in enumerate(self.prog.type_names) if n in set(static_types)], dtype=np.int32)
        if words_per_env is None:
            words_per_env = 4 * (K.RPL_STEP_WORDS + self.prog.max_objects * (1 + K.RPL_SLOT_WORDS) + K.RPL_END_WORDS)
        _check(self.L.mgx_set_replay(self.h, idx.ctypes.data, int(idx.size), int(words_per_env), tids.ctypes.data if tids.size else None,
                                     int(tids.size)))
        self.replay_envs = [int(x) for x in idx]

    def replay_layout(self) -> dict:
        out = np.zeros(len(self.RPL), np.int32)
        _check(self.L.mgx_replay_layout(self.h, out.ctypes.data))
        return {k: int(v) for k, v in zip(self.RPL, out)}

    def drain_replay(self):
        """(words, flags): per watched env, in watch-list order, the uint32 words logged since the last drain and the
        recorder's state bits (``K.RPL_ENV_OVERFLOW`` ...).  Empties the logs; waits for the device."""
        lay = self.replay_layout()
        n, cap = lay["NUM_ENVS"], lay["WORDS_PER_ENV"]
        if n == 0:
            raise ValueError("no watch list: set_replay(envs)")
        raw = np.empty((n, cap), np.uint32)
        used, flags = np.zeros(n, np.int32), np.zeros(n, np.uint32)
        _check(self.L.mgx_drain_replay(self.h, raw.ctypes.data, used.ctypes.data, flags.ctypes.data))
        return [raw[i, : used[i]].copy() for i in range(n)], [int(f) for f in flags]

    # ---- chosen stats after every step (include/mgx.h mgx_set_step_stats; csrc/mgx_step_stats.h) ----
    SSK = ("absent", "stat", "counter", "cov_unique", "cov_maxdist", "reward_step", "reward_episode", "steps")   # MGX_SSK_*

    def step_stat_columns(self, game_keys, agent_keys) -> tuple:
        """The column codes ``set_step_stats`` hands to the engine: per key the id of the program's game / agent stat table,
        ``K.SS_ABSENT`` for a name the table does not hold, or the code of a special key (host-only)."""
        gid = {n: i for i, n in enumerate(self.prog.game_stat_names)}
        aid = {n: i for i, n in enumerate(self.prog.agent_stat_names)}
        special_g = {"attributes/steps": K.SS_STEPS}
        special_a = {"reward_step": K.SS_REWARD_STEP, "reward_episode": K.SS_REWARD_EPISODE}
        g = [special_g[k] if k in special_g else gid.get(k, K.SS_ABSENT) for k in game_keys]
        a = [special_a[k] if k in special_a else aid.get(k, K.SS_ABSENT) for k in agent_keys]
        return np.asarray(g, dtype=np.int32), np.asarray(a, dtype=np.int32)

    def set_step_stats(self, game_keys, agent_keys) -> None:
        """From the next step on, a kernel behind every step writes the chosen stats of ALL envs and agents into four device
        tensors (``step_stats``) — what ``MettaGridPufferEnv(step_info_keys=...)`` reads after every ``sim.step()``
        (mettagrid_puffer_env.py:230-282).  ``game_keys``: names of game stats (``team/<t>/<s>`` keys are the game stats
        ``<t>/<s>``) or ``"attributes/steps"`` (the env's current step); ``agent_keys``: names of agent stats, ``"reward_step"``
        or ``"reward_episode"``.  At most 64 of each; two empty lists switch the readout off.  A name the compiled program's
        stat tables do not hold becomes an absent column (value 0, exists 0): the reference returns None for such a key and
        omits it.  The one known difference: ``action.invalid_index.<k>`` for k outside the fixed stat columns lives in the
        extras table (``invalid_index_extra``) and is reported as absent.  The tensors hold the LAST STEP's values: after
        ``reset_envs*`` / ``load_envs`` / ``copy_envs`` they are stale until the next step.  Device buffers only."""
        import torch
        game_keys, agent_keys = [str(k) for k in game_keys], [str(k) for k in agent_keys]
        if not game_keys and not agent_keys:
            _check(self.L.mgx_set_step_stats(self.h, None, 0, None, 0, None, None, None, None))
            self._step_stats, self.step_stat_keys = None, ([], [])
            return
        g, a = self.step_stat_columns(game_keys, agent_keys)
        dev = torch.device("cuda", self.device)
        rows = self.E * self.A
        t = (torch.zeros((self.E, g.size), dtype=torch.float32, device=dev), torch.zeros((self.E, g.size), dtype=torch.uint8, device=dev),
             torch.zeros((rows, a.size), dtype=torch.float32, device=dev), torch.zeros((rows, a.size), dtype=torch.uint8, device=dev))
        torch.cuda.synchronize(dev)   # (the engine's stream writes them from the next step on)
        ptr = [x.data_ptr() if x.numel() else None for x in t]
        _check(self.L.mgx_set_step_stats(self.h, g.ctypes.data if g.size else None, int(g.size), a.ctypes.data if a.size else None,
                                         int(a.size), *ptr))
        self._step_stats, self.step_stat_keys = t, (game_keys, agent_keys)   # (the old tensors are released only now)

    @property
    def step_stats(self):
        """(game f32 [E, KG], game_exists u8 [E, KG], agent f32 [E*A, KA], agent_exists u8 [E*A, KA]) of the last step, on the
        device and ordered on the engine's stream (``caller_waits``); None while no keys are set."""
        return getattr(self, "_step_stats", None)

    def step_stats_columns(self) -> tuple:
        """What the engine resolved each column to (``SSK`` names; include/mgx.h mgx_step_stats_columns): ``"counter"`` /
        ``"cov_unique"`` / ``"cov_maxdist"`` columns read the integer bookkeeping.  (game kinds, agent kinds)."""
        gk, ak = self.step_stat_keys if self.step_stats is not None else ([], [])
        out = np.zeros(len(gk) + len(ak), np.int32)
        _check(self.L.mgx_step_stats_columns(self.h, out.ctypes.data))
        names = [self.SSK[int(v)] for v in out]
        return names[:len(gk)], names[len(gk):]

    # ---- global state rows (include/mgx.h mgx_set_global_state; csrc/mgx_global_state.h; mettagrid_amd/global_state.py) ----
    def global_state_bound(self, exclude=()) -> int:
        """A row length no env of this engine can exceed when the classes in ``exclude`` (class ids, cell or type names such
        as ``"wall"``) are left out: from the program and the slot count (include/mgx.h mgx_global_state_bound)."""
        from .global_state import class_include
        inc = class_include(self.prog, exclude)
        out = C.c_int32(0)
        _check(self.L.mgx_global_state_bound(self.h, inc.ctypes.data, C.byref(out)))
        return out.value

    def set_global_state(self, max_tokens=None, exclude=(), agent_start: bool = True):
        """From now on a kernel behind every step writes the tokens of every object on every env's grid into device tensors,
        which are returned (and kept as ``global_state``): ``tokens`` uint32 [E, TG] (``row | col << 8 | feature << 16 |
        value << 24``; 0xFFFFFFFF behind an env's last token), ``counts`` uint32 [E] (untruncated: more than TG
        says the row overflowed) and ``agent_start`` int32 [E, A] (or None).  Format and order: ``mettagrid_amd/global_state.py``.
        ``max_tokens``: TG, default ``global_state_bound(exclude)``.  ``max_tokens=0`` switches the feature off.  The rows
        show the state after the last step; after ``reset_envs*`` / ``load_envs`` / ``copy_envs`` / ``set_inventory`` call
        ``write_global_state``.  Device buffers only."""
        import torch
        from .global_state import class_include
        if max_tokens is not None and int(max_tokens) == 0:
            _check(self.L.mgx_set_global_state(self.h, None, 0, None, None, None))
            self._global_state = None
            return None
        inc = class_include(self.prog, exclude)
        tg = self.global_state_bound(exclude) if max_tokens is None else int(max_tokens)
        if tg < 1:
            raise ValueError(f"set_global_state: max_tokens must be at least 1 (got {tg})")
        if self.kind != "device":
            raise ValueError("set_global_state: the engine is bound to host buffers; the rows need device buffers")
        dev = torch.device("cuda", self.device)
        t = (torch.empty((self.E, tg), dtype=torch.int32, device=dev).view(torch.uint32),
             torch.zeros(self.E, dtype=torch.int32, device=dev).view(torch.uint32),
             torch.full((self.E, self.A), -1, dtype=torch.int32, device=dev) if agent_start else None)
        self.bind_global_state(*t, include=inc)
        return self._global_state

    def bind_global_state(self, tokens, counts, agent_start=None, include=None) -> None:
        """``set_global_state`` with the caller's own contiguous device tensors (4-byte elements; ``tokens`` [E, TG])."""
        import torch
        torch.cuda.synchronize(torch.device("cuda", self.device))   # (the engine's stream writes them from now on)
        inc = None if include is None else np.ascontiguousarray(include, dtype=np.uint8)
        _check(self.L.mgx_set_global_state(self.h, tokens.data_ptr(), int(tokens.shape[-1]), counts.data_ptr(),
                                           agent_start.data_ptr() if agent_start is not None else None,
                                           inc.ctypes.data if inc is not None else None))
        self._global_state = (tokens, counts, agent_start)   # (the old tensors are released only now)

    @property
    def global_state(self):
        """(tokens, counts, agent_start) of ``set_global_state``, ordered on the engine's stream (``caller_waits``); None
        while the feature is off."""
        return getattr(self, "_global_state", None)

    def write_global_state(self, envs=None) -> None:
        """Rewrite the rows of ``envs`` (indices; None = all) from the current state, on the engine's stream: after
        ``reset_envs*``, ``load_envs``, ``copy_envs`` and ``set_inventory``, which leave them stale."""
        if envs is None:
            _check(self.L.mgx_write_global_state(self.h, None))
            return
        mask = np.zeros(self.E, np.uint8)
        mask[env_list(envs, self.E, "write_global_state")] = 1
        _check(self.L.mgx_write_global_state(self.h, mask.ctypes.data))

    @property
    def stream(self) -> int:
        return int(self.L.mgx_stream(self.h) or 0)

    # ---- ordering against the caller's torch stream (device buffers) ----
    def _ext_stream(self):
        import torch
        if getattr(self, "_ext", None) is None:
            self._ext = torch.cuda.ExternalStream(self.stream, device=torch.device("cuda", self.device))
        return self._ext

    def wait_for_caller(self) -> None:
        """Order the engine's stream behind everything the caller has enqueued on its current torch stream (the action
        writes): the engine's kernels then read the actions the caller meant."""
        import torch
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.device))
        self._ext_stream().wait_event(ev)

    def caller_waits(self) -> None:
        """Order the caller's current torch stream behind the engine's stream: tensors returned after ``step`` hold the
        step's results for any kernel the caller enqueues next (no host synchronisation)."""
        import torch
        ev = torch.cuda.Event()
        ev.record(self._ext_stream())
        torch.cuda.current_stream(self.device).wait_event(ev)

    def poll_errors(self):
        bits, first = C.c_uint32(0), C.c_int32(-1)
        _check(self.L.mgx_poll_errors(self.h, C.byref(bits), C.byref(first)))
        return bits.value, first.value

    def raise_env_errors(self) -> None:
        bits, first = self.poll_errors()
        if bits & ENV_TOKEN_OVERFLOW:  # reference: std::runtime_error -> RuntimeError (mettagrid_c.cpp:364-375)
            raise RuntimeError(f"Observation token budget exceeded (first env {first}, budget={self.T})")
        if bits & ENV_TOO_MANY_OBJECTS:
            raise MgxError(f"env {first}: map holds more objects than max_objects={self.prog.max_objects}")
        if bits & ENV_DEPTH:
            raise MgxError(f"env {first}: handler / inventory-limit recursion exceeds the engine's depth")
        if bits & ENV_INVALID_KEY_RANGE:
            raise MgxError(f"env {first}: an agent sent more than {K.INVALID_EXTRA} distinct invalid action indices far outside "
                           "the action table in one episode (action.invalid_index.<k> keys exhausted)")
        if bits & ENV_TOKEN_POOL:
            raise MgxError(f"env {first}: the observation kernel's per-env token cache is exhausted "
                           "(objects' token lists would be dropped from observations)")
        if bits & (ENV_PROXY_INVENTORY | ENV_AGENT_LIFECYCLE):
            raise MgxError(f"env {first}: a handler touched an agent's existence or a territory proxy's inventory (bits {bits})")

    # ---- readbacks ----
    def episode_rewards(self) -> np.ndarray:
        out = np.empty(self.E * self.A, np.float32)
        _check(self.L.mgx_get_episode_rewards(self.h, out.ctypes.data))
        return out

    def action_success(self) -> np.ndarray:
        out = np.empty(self.E * self.A, np.uint8)
        _check(self.L.mgx_get_action_success(self.h, out.ctypes.data))
        return out.astype(bool)

    def executed_actions(self) -> np.ndarray:
        """The action each agent executed in the last step (0: none succeeded), int32 [E*A] (mgx.h mgx_get_executed_actions)."""
        out = np.empty(self.E * self.A, np.int32)
        _check(self.L.mgx_get_executed_actions(self.h, out.ctypes.data))
        return out

    def invalidate_observations(self) -> None:
        """For callers that wrote into the bound observation buffer: the next observation pass rewrites whole rows
        (mgx.h mgx_invalidate_observations).  Between ``set_buffers`` calls the buffer otherwise belongs to the engine."""
        _check(self.L.mgx_invalidate_observations(self.h))

    def observation_counts(self) -> np.ndarray:
        """Tokens the last observation pass wrote into each row, u16 [E*A]; 0xFFFF = unknown (mgx.h)."""
        out = np.empty(self.E * self.A, np.uint16)
        _check(self.L.mgx_get_observation_counts(self.h, out.ctypes.data))
        return out

    def current_steps(self) -> np.ndarray:
        out = np.empty(self.E, np.uint32)
        _check(self.L.mgx_get_current_steps(self.h, out.ctypes.data))
        return out

    def raw_stats(self, env: int = 0):
        ng, na = len(self.prog.game_stat_names), len(self.prog.agent_stat_names)
        gv, gt = np.zeros(ng, np.float32), np.zeros(ng, np.uint8)
        av, at = np.zeros((self.A, na), np.float32), np.zeros((self.A, na), np.uint8)
        _check(self.L.mgx_get_stats(self.h, env, gv.ctypes.data, gt.ctypes.data, av.ctypes.data, at.ctypes.data))
        return gv, gt, av, at

    def invalid_index_extra(self, env: int = 0) -> list:
        """Per agent {k: count} of "action.invalid_index.<k>" for the k that have no fixed stat column (mgx.h)."""
        k = np.zeros((self.A, K.INVALID_EXTRA), np.int32)
        n = np.zeros((self.A, K.INVALID_EXTRA), np.float32)
        _check(self.L.mgx_get_invalid_index_extra(self.h, env, k.ctypes.data, n.ctypes.data))
        return [{int(k[a, q]): float(n[a, q]) for q in range(K.INVALID_EXTRA) if n[a, q] != 0} for a in range(self.A)]

    def get_episode_stats(self, env: int = 0) -> dict:
        return stats_dicts(self.prog, *self.raw_stats(env), extra=self.invalid_index_extra(env))

    def raw_objects(self, env: int = 0) -> np.ndarray:
        out = np.zeros((self.prog.max_objects, OBJ_RECORD_WORDS), np.int32)
        n = C.c_int32(0)
        _check(self.L.mgx_get_objects(self.h, env, out.ctypes.data, C.byref(n)))
        return out[: n.value]

    def raw_objects_batch(self, envs) -> list:
        """``raw_objects`` of many envs with one kernel and one device->host copy (include/mgx.h mgx_get_objects_batch)."""
        idx = np.ascontiguousarray(np.asarray(envs, dtype=np.int32).reshape(-1))
        if idx.size == 0:
            return []
        out = np.zeros((idx.size, self.prog.max_objects, OBJ_RECORD_WORDS), np.int32)
        n = np.zeros(idx.size, np.int32)
        _check(self.L.mgx_get_objects_batch(self.h, idx.ctypes.data, int(idx.size), out.ctypes.data, n.ctypes.data))
        return [out[i, : n[i]] for i in range(idx.size)]

    def grid_objects_batch(self, envs) -> list:
        """``grid_objects()`` dicts (cpp/bindings/mettagrid_py.cpp:28-139) of many envs; the per-agent reward state is still
        one small copy per env."""
        return [objects_from_raw(self.prog, raw, self.current_stat_reward(int(e)))
                for e, raw in zip(np.asarray(envs).reshape(-1), self.raw_objects_batch(envs))]

    def current_stat_reward(self, env: int = 0) -> np.ndarray:
        out = np.zeros(self.A, np.float32)
        _check(self.L.mgx_get_reward_state(self.h, env, out.ctypes.data))
        return out

    def grid_objects(self, env: int = 0) -> dict:
        return objects_from_raw(self.prog, self.raw_objects(env), self.current_stat_reward(env))

    def snapshot(self, env: int | None = None) -> dict:
        """Host copies of the caller-visible buffers (all envs, or the rows of one env)."""
        self.sync()
        if self.kind == "device":
            import torch
            torch.cuda.synchronize(self.device)
            obs, rew = self.obs.cpu().numpy(), self.rewards.cpu().numpy()
            term, trunc = self.terminals.cpu().numpy(), self.truncations.cpu().numpy()
        else:
            obs, rew, term, trunc = self.obs.copy(), self.rewards.copy(), self.terminals.copy(), self.truncations.copy()
        out = dict(obs=obs, rewards=rew, terminals=term.astype(bool), truncations=trunc.astype(bool),
                   action_success=self.action_success(), episode_rewards=self.episode_rewards())
        if env is not None:
            sl = slice(env * self.A, (env + 1) * self.A)
            out = {k: v[sl] for k, v in out.items()}
        return out

    def set_inventory(self, env: int, agent_id: int, inventory: dict) -> None:
        """``MettaGrid.set_inventory`` (cpp/bindings/mettagrid_py.cpp:203-207) for agent ``agent_id`` of env ``env``;
        ``inventory`` maps resource ids to amounts.  The reference walks the std::unordered_map pybind11 builds from
        the dict, so the items are applied in that map's iteration order (mettagrid_amd/umap.py)."""
        from .umap import from_pydict
        ids = [int(k) for k in inventory]
        order = from_pydict(ids).keys()
        items = np.asarray(order, dtype=np.int32)
        amounts = np.asarray([int(inventory[k]) for k in order], dtype=np.int32)
        _check(self.L.mgx_set_inventory(self.h, int(env), int(agent_id), items.ctypes.data, amounts.ctypes.data, len(order)))

    def count_objects_with_tag(self, env: int, tag_id: int) -> int:
        out = C.c_int32(0)
        _check(self.L.mgx_count_objects_with_tag(self.h, int(env), int(tag_id), C.byref(out)))
        return out.value

    def state_digests(self) -> np.ndarray:
        """uint64 [E]: digest of every env's signature state (objects, stats, rewards, success, step) in one kernel."""
        out = np.empty(self.E, np.uint64)
        _check(self.L.mgx_state_digests(self.h, out.ctypes.data))
        bits, first = self.poll_errors()
        if bits & 0x8000:  # MGX_ENV_INTERNAL: the digest kernel found a per-agent mirror out of step with its object row
            raise MgxError(f"env {first}: internal consistency check failed (per-agent mirror differs from the object row)")
        return out

    # ---- policy-side token decode ----
    def feature_scale(self) -> np.ndarray:
        """scale[f] = max(normalization of feature f, 1) (grid_obs_wrapper.py:39-44), from the compiled program."""
        scale = np.ones(256, np.float32)
        for i, z in enumerate(self.prog.feature_norms):
            scale[i] = max(float(z), 1.0)
        return scale

    def set_box_output(self, out=None):
        """Fused form of ``decode_obs`` (include/mgx.h mgx_set_box_output): from the next observation pass on the observation
        kernel writes the dense box of every agent into ``out`` — a contiguous torch CUDA tensor [E*A, C, H, W], float32
        (bit-identical to ``GridObsWrapper._convert``) or bfloat16 (that box rounded to nearest even) — instead of the token
        rows.  ``None`` switches back to token rows.  The tensor is kept alive here."""
        import torch
        if out is None:
            self._box = None
            _check(self.L.mgx_set_box_output(self.h, None, 0, 0, None))
            return
        Cn = len(self.prog.feature_norms)
        Hh, Ww = int(self.prog.words[K.H_OBS_HEIGHT]), int(self.prog.words[K.H_OBS_WIDTH])
        if tuple(out.shape) != (self.E * self.A, Cn, Hh, Ww) or out.dtype not in (torch.float32, torch.bfloat16) or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous float32 / bfloat16 tensor of shape {(self.E * self.A, Cn, Hh, Ww)}")
        scale = self.feature_scale()
        self._box = out
        _check(self.L.mgx_set_box_output(self.h, out.data_ptr(), 1 if out.dtype == torch.float32 else 2, Cn, scale.ctypes.data))

    def decode_obs(self, out=None, tokens=None):
        """Dense float32 box [rows, C, H, W] of the current observations (``GridObsWrapper._convert``), computed on the
        GPU and ordered on the engine's stream.  ``out``: torch CUDA tensor to fill (allocated if None); ``tokens``: another
        token tensor u8 [rows, T, 3] on the device instead of the engine's own observation buffer."""
        import torch
        Cn = len(self.prog.feature_norms)
        Hh, Ww = int(self.prog.words[K.H_OBS_HEIGHT]), int(self.prog.words[K.H_OBS_WIDTH])
        dev = torch.device("cuda", self.device)
        rows = self.E * self.A if tokens is None else int(tokens.shape[0])
        if out is None:
            out = torch.empty((rows, Cn, Hh, Ww), dtype=torch.float32, device=dev)
        if tuple(out.shape) != (rows, Cn, Hh, Ww) or out.dtype != torch.float32 or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous float32 tensor of shape {(rows, Cn, Hh, Ww)}")
        scale = self.feature_scale()
        tok_ptr = None
        if tokens is not None:
            if tokens.dtype != torch.uint8 or not tokens.is_contiguous() or tokens.shape[1:] != (self.T, 3):
                raise ValueError("tokens must be a contiguous uint8 tensor [rows, T, 3]")
            tok_ptr = tokens.data_ptr()
        _check(self.L.mgx_decode_obs(self.h, tok_ptr, rows, out.data_ptr(), Cn, scale.ctypes.data))
        return out

    def token_bag(self, out=None, counts=None, tokens=None, num_features=None):
        """Token-bag features of the current observations (include/mgx.h mgx_token_bag): ``(bag, counts)``,
        ``bag`` [rows, 32 + C] = per row the sums of ``value / (scale[feature] + 1e-6)`` by x nibble, by y nibble and by
        feature — everything ``token_bag.TokenBagEmbedding`` needs of a row — and ``counts`` int32 [rows], the row's tokens.
        Computed on the GPU, ordered on the engine's stream.  ``out``: contiguous float32 or bfloat16 CUDA tensor to fill
        (float32 allocated if None); ``counts``: contiguous int32 [rows]; ``tokens``: another token tensor u8 [rows, T, 3] on
        the device instead of the engine's own observation buffer; ``num_features``: C, default the program's feature count
        (tokens of a feature >= C are skipped and not counted)."""
        import torch
        Cn = len(self.prog.feature_norms) if num_features is None else int(num_features)
        if not 1 <= Cn <= 256:
            raise ValueError("num_features must be in [1, 256]")
        dev = torch.device("cuda", self.device)
        tok_ptr = None
        if tokens is not None:
            if (not isinstance(tokens, torch.Tensor) or tokens.dtype != torch.uint8 or tokens.ndim != 3 or tokens.shape[0] < 1
                    or tuple(tokens.shape[1:]) != (self.T, 3) or not tokens.is_contiguous() or tokens.device != dev):
                raise ValueError(f"tokens must be a contiguous uint8 tensor [rows >= 1, {self.T}, 3] on {dev}")
            tok_ptr = tokens.data_ptr()
        elif getattr(self, "_box", None) is not None:
            raise ValueError("token_bag: box output is on (set_box_output): the observation rows are not written")
        rows = self.E * self.A if tokens is None else int(tokens.shape[0])
        if out is None:
            out = torch.empty((rows, 32 + Cn), dtype=torch.float32, device=dev)
        if counts is None:
            counts = torch.empty((rows,), dtype=torch.int32, device=dev)
        if (not isinstance(out, torch.Tensor) or tuple(out.shape) != (rows, 32 + Cn) or out.dtype not in (torch.float32, torch.bfloat16)
                or not out.is_contiguous() or out.device != dev):
            raise ValueError(f"out must be a contiguous float32 / bfloat16 tensor of shape {(rows, 32 + Cn)} on {dev}")
        if (not isinstance(counts, torch.Tensor) or tuple(counts.shape) != (rows,) or counts.dtype != torch.int32
                or not counts.is_contiguous() or counts.device != dev):
            raise ValueError(f"counts must be a contiguous int32 tensor of shape {(rows,)} on {dev}")
        scale = self.feature_scale()
        _check(self.L.mgx_token_bag(self.h, tok_ptr, rows, out.data_ptr(), 1 if out.dtype == torch.float32 else 2, counts.data_ptr(), Cn,
                                    scale.ctypes.data))
        return out, counts

    # ---- rendering (include/mgx.h mgx_render_cells / mgx_set_render_tiles / mgx_render_rgb) ----
    @property
    def map_shape(self) -> tuple:
        return int(self.prog.words[K.H_HEIGHT]), int(self.prog.words[K.H_WIDTH])

    def render_cells(self, envs) -> np.ndarray:
        """The cell words of the listed envs (any order, repeats allowed), uint32 [n, H, W]: 0 for an empty cell, else
        ``(class + 1) | agent_id << 16 | vibe << 24`` (``mettagrid_amd/render.py``: ``ansi`` makes the reference's text frame
        of them, ``cells_from_objects`` the same words from ``grid_objects()``).  One kernel, one copy; a synchronous getter."""
        idx = env_list(list(envs) if not isinstance(envs, np.ndarray) else envs, self.E, "render_cells")
        H, W = self.map_shape
        out = np.empty((idx.size, H, W), np.uint32)
        _check(self.L.mgx_render_cells(self.h, idx.ctypes.data, int(idx.size), out.ctypes.data))
        return out

    def set_render_tiles(self, tiles=None, class_tile=None, agent_tile=None, vibe_rgb=None, scale=None) -> None:
        """The tile atlas ``render_rgb`` draws with: ``tiles`` uint8 [n_tiles, s, s, 3] (s in 1..32; tile 0: the empty cell),
        ``class_tile`` [classes] and ``agent_tile`` [A] tile indices, ``vibe_rgb`` uint8 [n_vibes, 3] or None (no vibe marker).
        ``set_render_tiles(scale=8)``: the atlas of ``render.default_tiles``.  ``set_render_tiles()``: frees the atlas."""
        from . import render
        if scale is not None:
            if tiles is not None:
                raise ValueError("set_render_tiles: give tiles or scale, not both")
            tiles, class_tile, agent_tile, vibe_rgb = render.default_tiles(self.prog, scale)
        if tiles is None:
            _check(self.L.mgx_set_render_tiles(self.h, None, 0, 0, None, None, None, 0))
            self.render_tiles = None
            return
        nc = int(self.prog.words[K.H_NUM_CLASSES])
        t = np.asarray(tiles)
        if t.dtype != np.uint8 or t.ndim != 4 or t.shape[0] < 1 or t.shape[0] > 65536 or t.shape[1] != t.shape[2] or t.shape[3] != 3:
            raise ValueError("set_render_tiles: tiles must be uint8 [1 <= n_tiles <= 65536, s, s, 3]")
        if not 1 <= t.shape[1] <= 32:
            raise ValueError(f"set_render_tiles: the tile size must be in [1, 32] (got {t.shape[1]})")
        if class_tile is None or agent_tile is None:
            raise ValueError("set_render_tiles: class_tile and agent_tile are needed")
        tables = []
        for name, tab, n in (("class_tile", class_tile, nc), ("agent_tile", agent_tile, self.A)):
            a = np.asarray(tab)
            if a.shape != (n,) or a.dtype.kind not in "iu":
                raise ValueError(f"set_render_tiles: {name} must hold {n} integers")
            if a.size and (a.min() < 0 or a.max() >= t.shape[0]):
                raise ValueError(f"set_render_tiles: {name} names a tile outside the atlas of {t.shape[0]} tiles")
            tables.append(np.ascontiguousarray(a, dtype=np.uint16))
        v = None
        if vibe_rgb is not None:
            v = np.asarray(vibe_rgb)
            if v.dtype != np.uint8 or v.ndim != 2 or v.shape[1] != 3 or not 1 <= v.shape[0] <= 256:
                raise ValueError("set_render_tiles: vibe_rgb must be uint8 [1 <= n_vibes <= 256, 3]")
            v = np.ascontiguousarray(v)
        t = np.ascontiguousarray(t)
        _check(self.L.mgx_set_render_tiles(self.h, t.ctypes.data, int(t.shape[0]), int(t.shape[1]), tables[0].ctypes.data, tables[1].ctypes.data,
                                           v.ctypes.data if v is not None else None, int(v.shape[0]) if v is not None else 0))
        self.render_tiles = (t, tables[0], tables[1], v)   # host copies: what render.rgb_host needs to restate a frame

    def render_rgb(self, envs, out=None):
        """RGB frames of the listed envs (any order, repeats allowed) on the device: uint8 CUDA tensor [n, H * s, W * s, 3], written
        on the engine's stream (``caller_waits`` orders the caller's stream behind it); every byte is written by every call.
        ``out``: a contiguous uint8 CUDA tensor with exactly that many elements to fill instead (any storage offset).  Needs
        ``set_render_tiles``."""
        import torch
        idx = env_list(list(envs) if not isinstance(envs, np.ndarray) else envs, self.E, "render_rgb")
        if getattr(self, "render_tiles", None) is None:
            raise ValueError("render_rgb: no atlas (set_render_tiles)")
        H, W = self.map_shape
        s = int(self.render_tiles[0].shape[1])
        shape = (int(idx.size), H * s, W * s, 3)
        dev = torch.device("cuda", self.device)
        if out is None:
            out = torch.empty(shape, dtype=torch.uint8, device=dev)
        if (not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or out.device != dev or not out.is_contiguous()
                or out.numel() != int(np.prod(shape))):
            raise ValueError(f"render_rgb: out must be a contiguous uint8 tensor of {int(np.prod(shape))} elements {shape} on {dev}")
        _check(self.L.mgx_render_rgb(self.h, idx.ctypes.data, int(idx.size), out.data_ptr()))
        return out.view(shape)

    def set_profiling(self, on: bool) -> None:
        _check(self.L.mgx_set_profiling(self.h, 1 if on else 0))

    TIMING_SEGMENTS = ("actions", "aoe", "tail", "obs", "rewards")   # include/mgx.h MGX_T_*

    def step_timing_segments_ms(self) -> dict:
        out = np.zeros(len(self.TIMING_SEGMENTS), np.float32)
        _check(self.L.mgx_get_step_timing(self.h, out.ctypes.data))
        return {k: float(v) for k, v in zip(self.TIMING_SEGMENTS, out)}

    def step_timing_ms(self):
        """(world update, observation + rewards) of the most recent step in milliseconds."""
        t = self.step_timing_segments_ms()
        return t["actions"] + t["aoe"] + t["tail"], t["obs"] + t["rewards"]

    @property
    def obs_variant(self) -> int:
        """0: generic observation kernel; 3: the instance compiled for the shape of BASELINE.json configs[2] (gen_presets.py);
        5: that shape with an episode length read at run time; 9: an instance compiled for this program at run time (jit.py)."""
        return int(self.L.mgx_obs_variant(self.h))

    @property
    def world_variant(self) -> int:
        """0: generic lean world kernel (shape read at run time); 3: the instance compiled for the shape of BASELINE.json
        configs[2] (gen_presets.py; never with MGX_NO_GEN or MGX_WORLD_GENERIC set at creation); 9: a code object compiled for
        this program at run time (jit.py)."""
        return int(self.L.mgx_world_variant(self.h))

    @property
    def handler_variant(self) -> int:
        """0: handler interpreter; 3 / 4: code generated at build() for the rung-3 / rung-4 preset (gen_handlers.py); 9: code
        generated for this program at run time (jit.py)."""
        return int(self.L.mgx_handler_variant(self.h))

    @property
    def act_variant(self) -> int:
        """0: action dispatch with one lane per env; 1: one lane per agent in conflict-ordered rounds (csrc/mgx_act.h)."""
        return int(self.L.mgx_act_variant(self.h))

    @property
    def dispatch_pairs(self) -> int:
        """1: the lean lane-per-env dispatch runs two agents of an env per trip where their footprints are disjoint."""
        return int(self.L.mgx_dispatch_pairs(self.h))

    @property
    def move_fast(self) -> int:
        """Non-zero: the lean kernel resolves move targets in its staging pass and runs trivial actions ahead (same results)."""
        return int(self.L.mgx_move_fast(self.h))

    def move_fast_counts(self) -> tuple:
        """(actions the run-ahead consumed, resolved entries found stale) over all envs and steps; needs env
        MGX_MOVE_FAST_COUNT at create, else (0, 0)."""
        out = (C.c_uint64 * 2)()
        _check(self.L.mgx_move_fast_counts(self.h, out))
        return int(out[0]), int(out[1])

    @property
    def integer_bookkeeping(self) -> int:
        """1: the per-action bookkeeping counters live as integers beside the stat rows (written into them before any read)."""
        return int(self.L.mgx_integer_bookkeeping(self.h))

    @property
    def paths(self) -> dict:
        """Every code path mgx_create chose for this program (include/mgx.h MGX_PATH_*): {name: bool}, names in
        PATH_BITS.  Diagnostic; the results are the same on either side of every entry."""
        bits = int(self.L.mgx_create_paths(self.h))
        return {name: bool(bits >> i & 1) for i, name in enumerate(PATH_BITS)}

    @property
    def state_bytes(self) -> int:
        return int(self.L.mgx_state_bytes(self.h))

    # ---- saving, loading and copying envs' state (include/mgx.h mgx_save_envs; DESIGN.md "Env state") ----
    def env_state_info(self) -> dict:
        info = EnvStateInfo()
        _check(self.L.mgx_env_state_info(self.h, C.byref(info)))
        return info.to_dict()

    def _box_check(self, what: str) -> None:
        if getattr(self, "_box", None) is not None:
            raise ValueError(f"{what}: box output is on (set_box_output): states hold observation rows")

    def save_envs(self, envs=None) -> EnvState:
        """Save the state of ``envs`` (default: all) into a new ``EnvState`` (device tensor; numpy for host engines).
        Ordered after everything enqueued before; the caller's stream waits for the copy."""
        lst = env_list(envs, self.E, "save_envs")
        self._box_check("save_envs")
        info = self.env_state_info()
        import torch
        buf = torch.empty((len(lst), info["record_bytes"]), dtype=torch.uint8, device=torch.device("cuda", self.device))
        if self.kind == "device":
            self.wait_for_caller()
        _check(self.L.mgx_save_envs(self.h, lst.ctypes.data, len(lst), C.c_void_p(buf.data_ptr())))
        if self.kind == "device":
            self.caller_waits()
            return EnvState(buf, info, lst)
        self.sync()
        return EnvState(buf.cpu().numpy(), info, lst)

    def load_envs(self, state: EnvState, envs=None) -> None:
        """Put the records of ``state`` into the slots ``envs`` (default: the slots they were saved from): each env then
        continues its saved episode bit for bit; its next episode is the slot's (seed, map pool schedule)."""
        lst = env_list(state.envs if envs is None else envs, self.E, "load_envs", unique=True)
        if len(lst) != len(state):
            raise ValueError(f"load_envs: {len(lst)} destination envs for {len(state)} records")
        self._box_check("load_envs")
        import torch
        data = state.data
        if isinstance(data, np.ndarray) or data.device != torch.device("cuda", self.device):
            data = torch.as_tensor(np.ascontiguousarray(data) if isinstance(data, np.ndarray) else data).to(
                torch.device("cuda", self.device))
        data = data.contiguous()
        if self.kind == "device":
            self.wait_for_caller()
        else:
            torch.cuda.synchronize(self.device)
        info = state.info_struct()
        _check(self.L.mgx_load_envs(self.h, lst.ctypes.data, len(lst), C.c_void_p(data.data_ptr()), C.byref(info)))
        self._keep_alive = data   # (read by the device after this returns)
        if self.kind == "device":
            self.caller_waits()

    def copy_envs(self, src, dst) -> None:
        """Copy the state of env ``src[k]`` onto env ``dst[k]``, as if every source were read before any destination
        is written (``[0, 1] -> [1, 0]`` swaps)."""
        s = env_list(src, self.E, "copy_envs")
        d = env_list(dst, self.E, "copy_envs", unique=True)
        if len(s) != len(d):
            raise ValueError(f"copy_envs: {len(s)} sources for {len(d)} destinations")
        self._box_check("copy_envs")
        if self.kind == "device":
            self.wait_for_caller()
        _check(self.L.mgx_copy_envs(self.h, s.ctypes.data, d.ctypes.data, len(s)))
        if self.kind == "device":
            self.caller_waits()


class MettaGrid:
    """One env with the reference's pybind surface (``MettaGrid(env_cfg, map, seed)``; here ``env_cfg`` is a compiled
    ``Program`` or a ``GameSpec``).  Buffers are caller-visible numpy arrays, stored by reference like the
    reference does (cpp/bindings/mettagrid_c.cpp:1165-1184): ``step()`` writes into them."""

    def __init__(self, env_cfg, map, seed: int, device: int = 0, buffers: str = "host") -> None:  # noqa: A002 - reference argument name
        """``buffers="device"``: the buffers are the engine's torch tensors instead (what the device-side features need, e.g.
        ``set_global_state``); ``set_buffers`` stays a host-array call."""
        H, W = len(map), len(map[0])
        prog = env_cfg if isinstance(env_cfg, Program) else compile_spec(env_cfg, H, W)
        self.prog = prog
        self._b = BatchedMettaGrid(prog, prog.class_map(map), [int(seed) & 0xFFFFFFFF], device=device, buffers=buffers)
        w = prog.words
        self.obs_width, self.obs_height = int(w[K.H_OBS_WIDTH]), int(w[K.H_OBS_HEIGHT])
        self.max_steps = int(w[K.H_MAX_STEPS])
        self.map_width, self.map_height = W, H
        self.object_type_names = list(prog.type_names)
        self.resource_names = list(prog.resource_names)
        self._num_agents = prog.num_agents
        self._profiling = False

    # -- buffers --
    def set_buffers(self, observations, terminals, truncations, rewards, actions, vibe_actions=None) -> None:
        n = self._num_agents
        if vibe_actions is None:
            vibe_actions = np.zeros(n, np.int32)
        want = ((observations, np.uint8), (terminals, np.bool_), (truncations, np.bool_), (rewards, np.float32),
                (actions, np.int32), (vibe_actions, np.int32))
        for arr, dt in want:  # pybind .noconvert(): dtype and C-contiguity are part of the signature
            if not isinstance(arr, np.ndarray) or arr.dtype != dt or not arr.flags.c_contiguous:
                raise TypeError("set_buffers(): incompatible function arguments (dtype / contiguity)")
        if observations.ndim != 3:
            raise RuntimeError(f"observations has {observations.ndim} dimensions but expected 3")
        if observations.shape[0] != n or observations.shape[2] != 3:
            raise RuntimeError(f"observations has shape {list(observations.shape)} but expected [{n}, [something], 3]")
        for name, arr in (("terminals", terminals), ("truncations", truncations), ("vibe_actions", vibe_actions),
                          ("rewards", rewards)):
            if arr.ndim != 1 or arr.shape[0] != n:
                raise RuntimeError(f"{name} has the wrong shape")
        b = self._b
        b.obs, b.terminals, b.truncations, b.rewards, b.actions, b.vibe_actions = (
            observations, terminals, truncations, rewards, actions, vibe_actions)
        b._bind(*(a.ctypes.data for a in (observations, terminals, truncations, rewards, actions, vibe_actions)),
                mem_kind=0, rows=observations.shape[0], tokens=observations.shape[1])

    def step(self) -> None:
        b = self._b
        if b.actions.ndim != 1:
            raise RuntimeError("actions must be 1D array")
        if b.actions.shape[0] != self._num_agents:
            raise RuntimeError("actions has the wrong shape")
        b.step(check_errors=True)

    def observations(self): return self._b.obs
    def terminals(self): return self._b.terminals
    def truncations(self): return self._b.truncations
    def rewards(self): return self._b.rewards
    def actions(self): return self._b.actions
    def vibe_actions(self): return self._b.vibe_actions

    def masks(self):
        return np.ones((self._num_agents, len(self.prog.action_names)), np.bool_)

    def get_episode_rewards(self): return self._b.episode_rewards()
    def get_episode_stats(self): return self._b.get_episode_stats(0)
    def action_success(self): return [bool(x) for x in self._b.action_success()]

    def get_game_stat(self, key: str):
        return self.get_episode_stats()["game"].get(key)

    def get_agent_stat(self, agent_id: int, key: str):
        st = self.get_episode_stats()["agent"]
        return st[agent_id].get(key) if 0 <= agent_id < len(st) else None

    @property
    def current_step(self) -> int:
        return int(self._b.current_steps()[0])

    def set_inventory(self, agent_id: int, inventory: dict) -> None:
        self._b.set_inventory(0, agent_id, inventory)

    def tag_index(self):
        from .mettagrid_c import TagIndex
        return TagIndex(self)

    # -- profiling properties (cpp/bindings/profiling_py.cpp:8-30); device time of the most recent step --
    def _timing(self) -> dict:
        if not self._profiling:
            self._b.set_profiling(True)
            self._profiling = True
            return {k: 0.0 for k in self._b.TIMING_SEGMENTS}
        try:
            return self._b.step_timing_segments_ms()
        except (MgxError, ValueError, RuntimeError):
            return {k: 0.0 for k in self._b.TIMING_SEGMENTS}

    @property
    def step_timing(self):
        """StepTimingStats: the fields of the reference's struct, filled from the engine's timing segments (a segment
        that covers several reference phases is reported under the first of them; see include/mgx.h MGX_T_*)."""
        t = self._timing()
        ns = {k: int(v * 1e6) for k, v in t.items()}
        from types import SimpleNamespace
        return SimpleNamespace(reset_ns=0, events_ns=0, actions_ns=ns["actions"], on_tick_ns=ns["tail"], aoe_ns=ns["aoe"],
                               observations_ns=ns["obs"], rewards_ns=ns["rewards"], truncation_ns=0, total_ns=sum(ns.values()))

    @property
    def last_obs_time_ns(self) -> int:
        return int(self._timing()["obs"] * 1e6)

    @property
    def obs_validation_stats(self):
        """The reference compares its two observation code paths when validation is compiled in; there is one path
        here, so the counters stay zero."""
        from types import SimpleNamespace
        return SimpleNamespace(comparison_count=0, mismatch_count=0, original_time_ns=0, optimized_time_ns=0)

    def grid_objects(self, min_row=-1, max_row=-1, min_col=-1, max_col=-1, ignore_types=()):
        objs = self._b.grid_objects(0)
        use_bounds = min_row >= 0 and max_row >= 0 and min_col >= 0 and max_col >= 0
        out = {}
        for oid, o in objs.items():
            if o["type_name"] in ignore_types:
                continue
            if use_bounds and not (min_row <= o["r"] < max_row and min_col <= o["c"] < max_col):
                continue
            out[oid] = o
        return out
