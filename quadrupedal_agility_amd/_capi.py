"""ctypes layer over the C ABI of include/*.h and the loader of the HIP library.

Nothing of the ABI is written down here: the constants, the Structure classes and every entry point's argtypes / restype are read from the
headers by _cdecl.py (tests/test_abi.py pins the result against the C compiler's layout and against tests/golden/abi.json).
The product path loads ONLY quadrupedal_agility_amd/csrc/libqa_sim.so (built by
__graft_entry__.build()).  It never falls back to a CPU path: a missing library raises.
"""
import ctypes as C
import os

import torch

from . import _cdecl as H

QA_ABI_VERSION = H.consts["QA_ABI_VERSION"]
(NUM_DOF, NUM_GAITS, NUM_PROP, HISTORY_LEN, NUM_OBS, NUM_OBS_DISC, ACTION_BUF_LEN, NUM_REWARDS, MOCAP_FRAME, MAX_MOCAP_CLIPS, MOCAP_CLIP, NUM_EXTRA_REWARDS,
 MAX_SCAN_POINTS) = H.values("QA_", "NUM_DOF NUM_GAITS NUM_PROP HISTORY_LEN NUM_OBS NUM_OBS_DISC ACTION_BUF_LEN NUM_REWARDS MOCAP_FRAME MAX_MOCAP_CLIPS "
                             "MOCAP_CLIP NUM_EXTRA_REWARDS MAX_SCAN_POINTS")
OBST_SEESAW, OBST_BAR, OBST_TYRE = H.values("QA_OBST_", "SEESAW BAR TYRE")
REWARD_NAMES = [n.lower() for n in H.names("QA_R_")]
# include/qa_sim_rewards.h: the terms qa_set_extra_rewards adds to the fused step, on caller-owned buffers
EXTRA_REWARD_NAMES = [n.lower() for n in H.names("QA_XR_")]
TENSORS = H.names("QA_T_")[:-1]                       # enum qa_tensor without its closing QA_T_COUNT
T = {name: i for i, name in enumerate(TENSORS)}
DTYPE_F32, DTYPE_I64, DTYPE_U8, DTYPE_I32, DTYPE_I16, DTYPE_F64 = H.values("QA_", "F32 I64 U8 I32 I16 F64")

# the Go2's bodies and joints in the engine's order (csrc/qa_go2_model.h): no header of include/ states it, so these two stay hand-written
BODY_NAMES = ["base", "Head_upper", "Head_lower"] + [
    f"{l}_{p}" for l in ("FL", "FR", "RL", "RR") for p in ("hip", "thigh", "calf", "foot")]
DOF_NAMES = [f"{l}_{p}_joint" for l in ("FL", "FR", "RL", "RR") for p in ("hip", "thigh", "calf")]
# include/qa_sim_reset.h (QA_BC_*): the body classes qa_set_contact_sets' masks are built from, and the kernels' defaults
BODY_CLASS_BITS = {n: H.consts["QA_BC_" + n.upper()] for n in ("base", "hip", "thigh", "calf", "foot")}
DEFAULT_TERMINATION_MASK, DEFAULT_PENALISED_MASK = H.values("QA_BC_DEFAULT_", "TERMINATION PENALISED")

RENDER_SHADOWS, RENDER_CHECKER, RENDER_ID_GROUND, RENDER_ID_CEILING, RENDER_ID_SKY, RENDER_AMBIENT, RENDER_CHECKER_SIZE, RENDER_CHECKER_DARK = H.values(
    "QA_RENDER_", "SHADOWS CHECKER ID_GROUND ID_CEILING ID_SKY AMBIENT CHECKER_SIZE CHECKER_DARK")
RENDER_SPHERE, RENDER_CAPSULE, RENDER_BOX = 0, 1, 2    # QA_RS_* kinds of csrc/qa_render_shapes.h, which is not a header of include/: hand-written
TSC_OBST_BAR, TSC_OBST_TYRE, TSC_OBST_STATE_WORDS = H.values("QA_TSC_OBST_", "BAR TYRE STATE_WORDS")
ADAM_STACK_MAX_TENSORS, ADAM_STACK_MAX_STATES = H.values("QA_ADAM_STACK_MAX_", "TENSORS STATES")
MLP_COPY, MLP_LAYER, MLP_GRAD, MLP_LOAD, MLP_MAX_OPS, MLP_MAX_OUTPUTS, MLP_F_SAVE, MLP_F_TRANSPOSED, MLP_F_ADD = H.values(
    "QA_MLP_", "COPY LAYER GRAD LOAD MAX_OPS MAX_OUTPUTS F_SAVE F_TRANSPOSED F_ADD")
# the activation codes of the policy chain: forward codes, and the codes of their derivatives (taken from the activation's output)
(MLP_ACT_NONE, MLP_ACT_ELU, MLP_ACT_RELU, MLP_ACT_TANH, MLP_ACT_LRELU, MLP_ACT_SELU, MLP_ACT_SIGMOID, MLP_ACT_ELU_GRAD, MLP_ACT_RELU_GRAD, MLP_ACT_TANH_GRAD,
 MLP_ACT_LRELU_GRAD, MLP_ACT_SELU_GRAD, MLP_ACT_SIGMOID_GRAD) = H.values(
    "QA_MLP_ACT_", "NONE ELU RELU TANH LRELU SELU SIGMOID ELU_GRAD RELU_GRAD TANH_GRAD LRELU_GRAD SELU_GRAD SIGMOID_GRAD")
MLP_BUF_COLS = H.values("QA_MLP_BUF", "0_COLS 1_COLS 2_COLS 3_COLS")
TSC_REWARD_NAMES = tuple(n.lower() for n in H.names("QA_TSC_REW_"))
# include/qa_tsc_rewards.h: the terms qa_tsc_goal_step_rewards adds to the goal step, on caller-owned buffers
TSC_EXTRA_REWARD_NAMES = tuple(n.lower() for n in H.names("QA_TSC_XR_"))
TSC_MAX_BODY_IDS = H.consts["QA_TSC_MAX_BODY_IDS"]
TSC_NUM_SCAN, TSC_NUM_OBS, TSC_NUM_OBS_BBC, TSC_NUM_OBS_DISC = H.values("QA_TSC_NUM_", "SCAN OBS OBS_BBC OBS_DISC")

QaConfig = H.struct("qa_config")
QaDiscSampleIo = H.struct("qa_disc_sample_io")
QaExtraRewards = H.struct("qa_extra_rewards")
QaTscDepthObstacles = H.struct("qa_tsc_depth_obstacles")
QaRenderCfg = H.struct("qa_render_cfg")
QaRenderIo = H.struct("qa_render_io")
QaTscObstCurr = H.struct("qa_tsc_obst_curr")
QaMlpOp = H.struct("qa_mlp_op")
QaWgradDesc = H.struct("qa_wgrad_desc")
QaPairJob = H.struct("qa_pair_job")
QaAdamPair = H.struct("qa_adam_pair")
QaAdamStackState = H.struct("qa_adam_stack_state")
QaAdamStackTensor = H.struct("qa_adam_stack_tensor")
QaTscGoalCfg = H.struct("qa_tsc_goal_cfg")
QaTscGoalIo = H.struct("qa_tsc_goal_io")
QaTscExtraRewards = H.struct("qa_tsc_extra_rewards")
QaTscObsCfg = H.struct("qa_tsc_obs_cfg")
QaTscObsIo = H.struct("qa_tsc_obs_io")
QaTscDepthCfg = H.struct("qa_tsc_depth_cfg")
QaTscDepthIo = H.struct("qa_tsc_depth_io")


def _field_names(cls, only=None):
    return tuple(name for name, ctype in cls._fields_ if only is None or ctype is only)


# the io blocks, whose every member is a pointer, and the pointers of qa_tsc_extra_rewards
RENDER_IO_FIELDS, TSC_GOAL_IO_FIELDS, TSC_OBS_IO_FIELDS, TSC_DEPTH_IO_FIELDS = (_field_names(c) for c in (QaRenderIo, QaTscGoalIo, QaTscObsIo, QaTscDepthIo))
TSC_EXTRA_POINTERS = _field_names(QaTscExtraRewards, only=C.c_void_p)

_HOST_ONLY = ("last_error", "abi_version")              # no oracle twin and no status to check: load_library sets their restype itself
ABI_SYMBOLS = [name for header, name, _, _ in H.prototypes if header == "qa_sim.h"]
# tests/golden/abi.json records the two lists, the Structure classes and the public constants of this module.  The headers named here have a
# record of their own beside it ({header: (record under tests/golden/, the header's structs)}; tools/abi_dump.py writes and checks both):
# their entry points are bound like every other (bind_extensions goes by the headers), their structs are read by the module that uses them.
_RECORDED_APART = {"qa_tsc_scan_obstacles.h": ("abi_scan_obstacles.json", ("qa_tsc_scan_obstacles",))}
# The same for the env engine's extension headers that came after abi.json was last written.  Their entry points are EXTENSION_SYMBOLS like those of
# the engine's other extension headers; tools/abi_dump.py keeps them out of abi.json's record and writes / checks the record named here.
_RECORDED_APART_ENGINE = {"qa_sim_actuators.h": ("abi_actuators.json", ("qa_actuators",))}
EXTENSION_SYMBOLS = [name for header, name, _, _ in H.prototypes if header != "qa_sim.h" and header not in _RECORDED_APART]


def _bind(lib, prefix, extension):
    for header, name, restype, argtypes in H.prototypes:
        if (header != "qa_sim.h") == extension and name not in _HOST_ONLY:
            f = getattr(lib, prefix + name)
            f.argtypes, f.restype = argtypes, restype
    return lib


def bind(lib, prefix):
    """Declare argtypes/restypes of the C ABI of include/qa_sim.h on a loaded library whose
    symbols carry `prefix` (the product library uses "qa_")."""
    return _bind(lib, prefix, False)


def bind_extensions(lib, prefix="qa_"):
    """Entry points declared in the extension headers next to include/qa_sim.h (EXTENSION_SYMBOLS and those of _RECORDED_APART*): exported by
    the HIP library only, no oracle twin, not part of ABI_SYMBOLS."""
    return _bind(lib, prefix, True)


_LIB = None
# QA_LIB: another build of the SAME library (A/B measurements of a kernel variant, tools/r5_call.sh); there is still no fallback -- a missing file raises
LIB_PATH = os.environ.get("QA_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "libqa_sim.so")


def load_library():
    """Load the HIP library; raise loudly if it has not been built (no CPU fallback exists)."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950). quadrupedal_agility_amd has no CPU fallback.")
        # PyTorch ships its own HIP runtime (torch/lib/libamdhip64.so); the device pointers and streams this library is
        # handed belong to THAT runtime.  torch is imported at the top of this module, so our DT_NEEDED libamdhip64 resolves to
        # the copy already in the process -- loaded the other way round, the process holds two runtimes and ours sees no device.
        lib = C.CDLL(LIB_PATH)
        bind(lib, "qa_")
        bind_extensions(lib, "qa_")
        lib.qa_last_error.restype = C.c_char_p
        lib.qa_abi_version.restype = C.c_int
        if lib.qa_abi_version() != QA_ABI_VERSION:
            raise RuntimeError("libqa_sim.so ABI version mismatch")
        _LIB = lib
    return _LIB


def tensor_info(lib, prefix, cfg, which):
    off = C.c_int64(); shape = (C.c_int64 * 3)(); nd = C.c_int32(); dt = C.c_int32()
    rc = getattr(lib, prefix + "tensor_info")(C.byref(cfg), which, C.byref(off), shape, C.byref(nd), C.byref(dt))
    if rc != 0:
        raise RuntimeError(f"{prefix}tensor_info({which}) -> {rc}")
    return off.value, tuple(shape[i] for i in range(nd.value)), dt.value


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def stream(on):
    """the CURRENT stream of a torch.device, or of a tensor's device, as the C ABI takes it; None on the CPU (the oracle's twins ignore it)"""
    dev = on if type(on) is torch.device else on.device
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream) if dev.type == "cuda" else None


NO_ERROR_TEXT = "(an injected library: no error text)"


class Api:
    """The one way to call an entry point of include/qa_sim.h from Python: `API.launch("slab_sum", ..., on=tensor)` appends the current stream
    of `on`, `API.call("set_lean_exports", ...)` appends nothing; both raise RuntimeError on a non-zero status.  `lib` / `prefix` inject another
    library exporting the same entry points under another prefix (the tests pass the oracle's twins); the default is libqa_sim.so, loaded at the
    first use, and it is required.  Entry points that return a COUNT (`*_scratch_bytes`, `arena_bytes`, `mlp_strands`, ...) are called on
    `fn(name)` / `lib` directly: they have no status to check."""

    stream = staticmethod(stream)

    def __init__(self, lib=None, prefix="qa_"):
        self._lib, self.prefix = lib, prefix
        self._fns = {}

    @property
    def lib(self):
        if self._lib is None:
            self._lib = load_library()
        return self._lib

    def fn(self, name):
        f = self._fns.get(name)
        if f is None:
            f = self._fns[name] = getattr(self.lib, self.prefix + name)
        return f

    def check(self, name, rc):
        """the status check itself, for a site that has to look at the code (or tidy up) before it raises"""
        if rc != 0:
            last = getattr(self.lib, self.prefix + "last_error", None)
            text = last() if last is not None else NO_ERROR_TEXT
            raise RuntimeError(f"{self.prefix}{name} failed with code {rc}: {text.decode() if isinstance(text, bytes) else text}")

    def call(self, name, *args):
        rc = self.fn(name)(*args)
        if rc != 0:
            self.check(name, rc)

    def launch(self, name, *args, on):
        rc = self.fn(name)(*args, stream(on))
        if rc != 0:
            self.check(name, rc)


API = Api()

_scratch = {}


def scratch_for(dev, nbytes, floor=0):
    """A scratch buffer of at least `nbytes` for a launch on the current stream of `dev`, kept per device AND stream (two launches on two
    streams must not share partial sums) and per `floor` (the size a new buffer has at least: each caller keeps its own buffer and sizing)."""
    if torch.cuda.is_current_stream_capturing():
        # a recording bakes the address in: the buffer must belong to the graph's pool, never to a cache whose buffer a later, larger request
        # replaces -- the old block would go back to the allocator and the replays would write partial sums into freed memory
        return torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
    key = (dev, torch.cuda.current_stream(dev).cuda_stream, floor)
    buf = _scratch.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = _scratch[key] = torch.empty(max(nbytes, floor), dtype=torch.uint8, device=dev)
    return buf
