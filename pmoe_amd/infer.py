"""Closed-loop inference helper (reference caller ``autoagents/image_agent.py:127-177``).

At B=1 the eval-mode forward is ~150 small launches and the tick time is launch latency, not kernel time.  The engine
allocates only through torch's caching allocator and (in eval mode) never synchronises with the host, so the whole
chain can be captured ONCE into a HIP graph (``torch.cuda.CUDAGraph`` is hipGraph on ROCm) and replayed per tick with
new inputs copied into the captured input buffers.  Parameters are read through the captured packed-weight buffers; every
replay first compares the engine's build / pointer-table / version keys with those taken at capture and re-captures
(:meth:`GraphedMixture.refresh`) when a weight, a BatchNorm buffer, the compute dtype or the device has changed since.

:class:`PolicyTick` is the agent's loop for every model type (frame and mask history on the device, the draw on the device);
:class:`AgentStep` is the whole ``run_step`` around it (``image_agent.py:114-177``): the camera's BGRA bytes, the speed and the
command in, (steer, throttle, brake) out.
"""
import types

import numpy as np
import torch

from . import hip, ops
from .engine import r16
from .preprocess import _coeffs
from .model import moe as _moe
from .model.moe import MixtureDistribution


class _RecordedChain:
    """``fn()`` -- an eval-mode launch chain on fixed buffers -- warmed up twice (packs weights, builds pointer tables: cached on the
    parameters' versions), then run once more and kept: captured into a HIP graph (``graph=True``; warm-up on a side stream, as
    capture asks), or recorded launch by launch (``hip.LaunchRecorder``) while allocating from a private ``torch.cuda.MemPool``
    that lives as long as this object, so every recorded pointer stays valid and nothing else is handed that memory.
    ``replay()`` issues the chain again (a plan: on the stream it was recorded on) and returns what ``fn`` returned."""

    def __init__(self, fn, graph=False):
        self.pool = None
        with torch.no_grad():
            if graph:
                side = torch.cuda.Stream()
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    for _ in range(2):
                        fn()
                torch.cuda.current_stream().wait_stream(side)
                self.runner = torch.cuda.CUDAGraph()
                with torch.cuda.graph(self.runner):
                    self.result = fn()
            else:
                for _ in range(2):
                    fn()
                self.pool = torch.cuda.MemPool()
                with torch.cuda.use_mem_pool(self.pool), hip.LaunchRecorder() as self.runner:
                    self.result = fn()

    def replay(self):
        self.runner.replay()
        return self.result


class _StaticMixture:
    """``model.mixture_params`` for inputs of one shape, kept as a :class:`_RecordedChain` and replayed per tick with the new inputs
    copied into the chain's input buffers.  Every call first compares the engine's ``replay_key()`` with the one taken when the
    chain was made and makes it again (:meth:`refresh`) when a weight, a BatchNorm buffer, the compute dtype or the device has
    changed since, or an eager call in between re-packed or re-allocated what the chain points to."""
    _graph, _verb, _done = False, "records", "recorded"

    def __init__(self, model, images, speed, command):
        if model.training:
            raise RuntimeError(f"{type(self).__name__} {self._verb} the eval-mode chain: call model.eval() first")
        self._check_inputs(images, speed, command)
        self.model = model
        self.static_in = [images.clone(), speed.clone(), command.clone()]
        self.refresh()

    def _check_inputs(self, *inputs):
        pass

    def refresh(self):
        """(re)capture / (re)record -- after load_state_dict / parameter updates."""
        self.chain = _RecordedChain(lambda: self.model.mixture_params(*self.static_in), self._graph)
        self.static_out = self.chain.result
        self.key = self.model._engine().replay_key()

    def __call__(self, images, speed, command):
        for dst, src in zip(self.static_in, (images, speed, command)):
            if dst.shape != src.shape:
                raise ValueError(f"{type(self).__name__} was {self._done} for input shape {tuple(dst.shape)}, got {tuple(src.shape)}")
            dst.copy_(src)
        if self.model._engine().replay_key() != self.key:
            self.refresh()
        return self.chain.replay()

    def sample(self, images, speed, command):
        probs, mean, std, _ = self(images, speed, command)
        return MixtureDistribution(probs, mean, std).sample()


class GraphedMixture(_StaticMixture):
    """``gm = GraphedMixture(model, images, speed, command)`` captures ``model.mixture_params`` for inputs of that shape;
    ``gm(images, speed, command)`` -> (probs, mean, std, speeds) and ``gm.sample(...)`` -> actions ``[B,2]`` replay it."""
    _graph, _verb, _done = True, "captures", "captured"
    graph = property(lambda self: self.chain.runner)


class PlannedMixture(_StaticMixture):
    """The same tick WITHOUT graph capture: the launches of one eval-mode ``model.mixture_params`` call are recorded once
    (``hip.LaunchRecorder``: C-ABI function + its converted arguments, descriptors included) and re-issued per tick straight
    through ctypes -- none of the engine's Python (shape logic, descriptor filling, allocation, pointer validation) runs
    again.  Same contract as :class:`GraphedMixture`: fixed input shapes, ``refresh()`` after a weight change, replay on the
    stream the plan was recorded on.  Inputs must already be float32 and contiguous (then the chain contains no torch kernel,
    only library launches)."""
    plan = property(lambda self: self.chain.runner)
    pool = property(lambda self: self.chain.pool)

    def _check_inputs(self, *inputs):
        for t in inputs:
            if t.dtype != torch.float32 or not t.is_contiguous():
                raise ValueError("PlannedMixture: inputs must be contiguous float32 tensors")


class PolicyTick:
    """The agent's loop (``autoagents/image_agent.py:127-177``) for EVERY model type ``get_model`` returns: the object keeps what
    the agent keeps -- the last T frames, and for PU-Net models the masks ``unet`` made of them -- on the device, and
    ``tick(frame, speed, command)`` -> actions ``[B,2]`` means ``model.sample(stack of the last T frames, speed, command)`` in
    eval mode.  Per tick:

    * one ``pmoe_history_push`` moves the frame ring ``[B,T,3,H,W]`` (what the mixture's stem reads) and writes the new frame
      as the NHWC tensor ``unet`` takes;
    * PU-Net models run ``PUNetEngine.forward_cached``: ONE ``unet`` pass (the newest frame; the other T - 1 masks are last
      ticks' outputs, bit for bit, because eval-mode BatchNorm makes a mask a function of its frame alone), a second push for
      the mask ring, then the F roll-out steps, backbone and heads;
    * mixtures run ``mixture_params`` and ``pmoe_mixture_draw`` (device-side draw from a counter kept in device memory; for
      ``PMoE`` the same launch blends the draw with the PU-Net expert's actions).

    ``mode="eager"`` runs the engine's Python every tick; ``mode="plan"`` records these launches once (``hip.LaunchRecorder``,
    private ``torch.cuda.MemPool``) and re-issues them through ctypes, all on one stream.  ``tick`` returns the object's own
    output buffer (copy it to keep it across ticks); ``tick.last`` holds the deterministic tensors of the most recent tick:
    ``probs, mean, std, speeds`` (mixtures), ``punet_actions, pred_speed`` (PU-Net models), ``raw`` (the draw), else None.
    A weight / BatchNorm-buffer / compute-dtype / device change is noticed on the next tick (``replay_key``): the plan is
    re-recorded and all T masks are recomputed from the frame history."""

    def __init__(self, model, batch=1, height=224, width=224, mode="plan", seed=0):
        if mode not in ("eager", "plan"):
            raise ValueError(f"PolicyTick: mode must be 'eager' or 'plan', got {mode!r}")
        if model.training:
            raise RuntimeError("PolicyTick runs the eval-mode chain: call model.eval() first")
        if isinstance(model, _moe.PMoE):
            self.moe, self.pun = model.moe, model.punet
        elif isinstance(model, _moe.PUNetExpert):
            self.moe, self.pun = None, model
        elif hasattr(model, "mixture_params"):
            self.moe, self.pun = model, None
        else:
            raise TypeError(f"PolicyTick: {type(model).__name__} is not a model type of get_model")
        if batch < 1 or height < 1 or width < 1:
            raise ValueError("PolicyTick: batch, height and width must be positive")
        if self.pun is not None and (height % 16 or width % 16):
            raise ValueError("PolicyTick: the U-Nets need a height and width divisible by 16")
        self.model, self.mode = model, mode
        self.B, self.H, self.W = int(batch), int(height), int(width)
        main = self.moe if self.moe is not None else self.pun
        eng = main._engine()
        self.T = self.pun.punet.n_past_frames if self.pun is not None else eng.conv1.cin // 3
        if self.moe is not None and self.moe._engine().conv1.cin != 3 * self.T:
            raise ValueError("PolicyTick: the mixture and the PU-Net expert look at different numbers of past frames")
        n_speed, n_cmd = eng.speed_enc["layers"][0].cin, eng.cmd_enc["layers"][0].cin
        # ---- everything below touches the device
        dev = next(model.parameters()).device
        if dev.type != "cuda":
            raise RuntimeError(f"PolicyTick: the model is on {dev}; pmoe_amd has no CPU path")
        hip.load()
        f32 = torch.float32
        with torch.cuda.device(dev):
            self.frames = torch.zeros(self.B, self.T, 3, self.H, self.W, dtype=f32, device=dev)
            self.static_in = [torch.zeros(self.B, 3, self.H, self.W, dtype=f32, device=dev),
                              torch.zeros(self.B, n_speed, dtype=f32, device=dev), torch.zeros(self.B, n_cmd, dtype=f32, device=dev)]
            self.state = torch.zeros(2, dtype=torch.int64, device=dev)
            self.raw = torch.zeros(self.B, 2, dtype=f32, device=dev)
            self.out = torch.zeros(self.B, 2, dtype=f32, device=dev)
        self.masks = self.newest = None
        self.plan = self.pool = self.key = None
        self.last = types.SimpleNamespace(probs=None, mean=None, std=None, speeds=None, punet_actions=None, pred_speed=None,
                                          raw=None)
        self.reseed(seed)
        self.reset()

    # ------------------------------------------------------------------ state
    def _key(self):
        """what a recorded tick (and, in either mode, the cached masks) depend on beyond this object's own buffers"""
        key = []
        for m in (self.pun, self.moe):
            if m is not None:
                key.append((m.dtype_in_use(), bool(m.fp8_weights), m._engine().replay_key()))
        if self.moe is not None and self.pun is not None:
            key.append(tuple(p.data_ptr() for l in (self.model.lat_weights, self.model.long_weights) for p in (l.weight, l.bias)))
        return tuple(key)

    def reseed(self, seed):
        """rewrite the device-resident draw state {seed, draws_done = 0}"""
        seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.state.copy_(torch.tensor([seed - (1 << 64) if seed >> 63 else seed, 0], dtype=torch.int64))

    @property
    def draws_done(self):
        """the draw counter, read back from the device (synchronises)"""
        return int(self.state[1].item())

    def reset(self):
        """start of an episode: T zero frames (image_agent.py:63-64); PU-Net models: ``unet(0)`` once, in every mask slot"""
        self.frames.zero_()
        if self.key is None or self._key() != self.key:
            self.refresh()
        elif self.pun is not None:
            with torch.no_grad():
                self.newest.zero_()
                m = self.pun._engine().mask_of(self.frames, self.newest, self.pun.dtype_in_use())
                for t in range(self.T):
                    self.masks[0, t].copy_(m)

    def refresh(self):
        """(re)build: packs and shadows, ALL T masks from the frame history (masks of other weights are stale), and in plan mode
        the recording.  Runs by itself when the engines' plan key has changed."""
        dev = next(self.model.parameters()).device
        if dev != self.frames.device:            # the model moved: this object's buffers follow it
            self._follow(dev)
        with torch.no_grad(), torch.cuda.device(dev):
            if self.pun is not None:
                eng, dtype, _ = self.pun.resolve_engine()
                pu = self.pun.punet
                if self.masks is None or self.masks.dtype != dtype:
                    self.masks = torch.zeros(1, self.T, self.B, self.H, self.W, r16(pu.num_classes), dtype=dtype, device=dev)
                    self.newest = torch.zeros(self.B, self.H, self.W, r16(pu.in_features), dtype=dtype, device=dev)
                eng.prepare(self.frames, dtype)
                for t in range(self.T):
                    ops.nchw_to_nhwc(self.frames[:, t].contiguous(), self.newest)
                    self.masks[0, t].copy_(eng.mask_of(self.frames, self.newest, dtype))
            if self.moe is not None:             # banks, pointer tables and packs of the mixture: what its half of the key reads
                eng, dtype, _ = self.moe.resolve_engine()
                eng.prepare(self.frames, dtype)
            self.plan = self.pool = None
            if self.mode == "plan":
                # the recorded run (and its warm-up, which packs weights and folds BatchNorms: cached on the parameters' versions)
                # moves the rings and the draw counter like any tick: put them back afterwards
                saved = [t.clone() for t in (self.frames, self.state) + ((self.masks,) if self.masks is not None else ())]
                chain = _RecordedChain(self._body)
                self.plan, self.pool, self._result = chain.runner, chain.pool, chain.result
                for dst, src in zip((self.frames, self.state, self.masks), saved):
                    dst.copy_(src)
            self.key = self._key()

    def _follow(self, dev):
        self.frames, self.state, self.raw, self.out = (t.to(dev) for t in (self.frames, self.state, self.raw, self.out))
        self.static_in = [t.to(dev) for t in self.static_in]
        self.masks = self.newest = None

    # ------------------------------------------------------------------ one tick
    def _push(self):
        """the first launch of a tick: the new frame into the ring (and, for the U-Nets, into ``newest``)"""
        ops.history_push(self.frames, self.static_in[0], nhwc=self.newest)

    def _body(self):
        """the launches of one tick, in order: frame push, PU-Net expert (its mask push inside), mixture, draw (+ blend)"""
        _, speed, command = self.static_in
        res = dict(probs=None, mean=None, std=None, speeds=None, punet_actions=None, pred_speed=None, raw=None)
        self._push()
        if self.pun is not None:
            eng, dtype, _ = self.pun.resolve_engine()
            res["punet_actions"], res["pred_speed"] = eng.forward_cached(self.frames, self.newest, self.masks, speed, command, dtype)
            actions = res["punet_actions"]
        if self.moe is not None:
            res["probs"], res["mean"], res["std"], res["speeds"] = self.moe.mixture_params(self.frames, speed, command)
            blend = None
            if self.pun is not None:
                m = self.model
                blend = (m.lat_weights.weight, m.lat_weights.bias, m.long_weights.weight, m.long_weights.bias)
            ops.mixture_draw(res["probs"], res["mean"], res["std"], self.state, self.raw, res["punet_actions"], blend,
                             self.out if blend is not None else None)
            res["raw"] = self.raw
            actions = self.out if blend is not None else self.raw
        return actions, res

    def tick(self, frame, speed, command):
        """frame f32 [B,3,H,W] (contiguous, on the device), speed [B,1], command [B,n_commands] -> actions [B,2] f32"""
        if self.model.training:
            raise RuntimeError("PolicyTick runs the eval-mode chain: call model.eval() first")
        for dst, src, name in zip(self.static_in, (frame, speed, command), ("frame", "speed", "command")):
            if tuple(dst.shape) != tuple(src.shape):
                raise ValueError(f"PolicyTick: {name} must be {tuple(dst.shape)}, got {tuple(src.shape)}")
            dst.copy_(src)
        self._fresh()
        return self._issue()

    def _fresh(self):
        if self._key() != self.key:              # weights / buffers / dtype / device changed: cached masks and the plan are stale
            self.refresh()

    def _issue(self):
        """the launches of one tick on what the input buffers hold"""
        with torch.no_grad():
            if self.plan is not None:
                self.plan.replay()
                actions, res = self._result
            else:
                actions, res = self._body()
        self.last = types.SimpleNamespace(**res)
        return actions

    __call__ = tick


class _SensorTick(PolicyTick):
    """the tick inside an :class:`AgentStep`: its first launch reads the camera's bytes, its last one writes the control"""

    def __init__(self, agent, model, **kw):
        self.agent = agent
        super().__init__(model, **kw)

    def refresh(self):
        dev = next(self.model.parameters()).device
        if dev != self.frames.device:
            self._follow(dev)
        self.agent._device_buffers(self, dev)    # (before the recording: the plan keeps their pointers)
        super().refresh()

    def _push(self):
        a = self.agent
        ops.sensor_push(a._frame_dev, self.frames, a.top, a.rows, a._htable, a._vtable, a.tile, nhwc=self.newest)

    def _body(self):
        actions, res = super()._body()
        ops.control_postprocess(actions, self.agent._control_dev)
        return actions, res


class AgentStep:
    """``run_step`` of the agent (``autoagents/image_agent.py:114-177``) as one object: ``agent.step(bgra, spd, cmd)`` takes what
    CARLA hands over -- the camera's uint8 BGRA frame ``[H0,W0,4]`` (numpy or CPU tensor; ``[B,H0,W0,4]`` for a batch), the speed
    (a float, or B of them) and the waypointer's ``RoadOption`` value (an int, or B) -- and returns float64 numpy ``[B,3]`` =
    (steer, throttle, brake), the numbers of a ``carla.VehicleControl``.

    It holds a :class:`PolicyTick` (``agent.tick``; ``reset()``, ``reseed()``, ``last`` and ``draws_done`` are the tick's) whose
    first launch is ``pmoe_sensor_push`` -- Crop -> Resize -> ToTensor straight from the BGRA bytes into the frame ring, bit-exact
    with the PIL chain -- and whose last one is ``pmoe_control_postprocess``.  Per step: the frame goes into one pinned uint8
    buffer, speed / ``speed_factor`` (divided in double, rounded to f32 once) and the one-hot command (index ``cmd - 1``, or 3
    when that is negative) into one pinned f32 buffer, two non-blocking uploads, the plan (``mode="eager"``: the same launches
    through the engine's Python), one 24 B download per batch row, one event wait.  Nothing is allocated per step; the
    coefficient tables are built once.  Weight, buffer, dtype and device changes are noticed like the tick notices them.

    ``log``: a :class:`pmoe_amd.vision.FrameLog` of the step's size and device (anything else is a ``ValueError`` here) keeps the
    reference's video log (``image_agent.py:162-173``: ``draw_on_image(rgb, measurements, action, False)`` per tick): after the
    tick's launches and before the control download, ``step()`` itself issues one ``log.push`` on the same stream -- the newest
    ring slot, the tick's action, the speed and one-hot command views -- so the recorded plan is the same with and without a
    log.  With ``log=None`` there is no launch and nothing else differs."""

    def __init__(self, model, sensor=(600, 800), crop=(125, 90), size=(224, 224), batch=1, mode="plan", seed=0, speed_factor=10.0,
                 log=None):
        if mode not in ("eager", "plan"):
            raise ValueError(f"AgentStep: mode must be 'eager' or 'plan', got {mode!r}")
        if log is not None:
            from .vision import FrameLog
            if not isinstance(log, FrameLog):
                raise TypeError("AgentStep: log is a pmoe_amd.vision.FrameLog")
            if log.size != (int(size[0]), int(size[1])):
                raise ValueError(f"AgentStep: the FrameLog holds {log.size} frames, the step makes {tuple(size)} ones")
            if log.capacity < batch:
                raise ValueError(f"AgentStep: a FrameLog of capacity {log.capacity} cannot take {batch} frames per step")
        if model.training:
            raise RuntimeError("AgentStep runs the eval-mode chain: call model.eval() first")
        self.H0, self.W0 = int(sensor[0]), int(sensor[1])
        self.top, self.bottom = int(crop[0]), int(crop[1])
        self.rows = self.H0 - self.top - self.bottom
        h, w = int(size[0]), int(size[1])
        if self.top < 0 or self.bottom < 0 or self.rows < 1 or self.W0 < 1:
            raise ValueError(f"AgentStep: crop ({self.top}, {self.bottom}) leaves no rows of a {self.H0} x {self.W0} frame")
        if batch < 1 or h < 1 or w < 1:
            raise ValueError("AgentStep: batch and size must be positive")
        self.model, self.B, self.speed_factor = model, int(batch), float(speed_factor)
        self._hcoeffs, self._vcoeffs = _coeffs(self.W0, w), _coeffs(self.rows, h)
        self.tile = ops.sensor_tile(self._vcoeffs[1], w)
        self._frame_dev = self._control_dev = self._meas_dev = self._htable = self._vtable = None
        self.tick = _SensorTick(self, model, batch=self.B, height=h, width=w, mode=mode, seed=seed)
        if log is not None and log.device != self.tick.frames.device:
            raise ValueError(f"AgentStep: the FrameLog is on {log.device}, the model on {self.tick.frames.device}")
        self.log = log
        # ---- the host side of a step: pinned, written in place
        self._frame_host = torch.empty(self.B, self.H0, self.W0, 4, dtype=torch.uint8, pin_memory=True)
        self._meas_host = torch.zeros(self._meas_dev.numel(), dtype=torch.float32, pin_memory=True)
        self._control_host = torch.zeros(self.B, 3, dtype=torch.float64, pin_memory=True)
        self._frame_np, self._meas_np, self._control_np = (t.numpy() for t in (self._frame_host, self._meas_host, self._control_host))
        self._done = torch.cuda.Event()

    _ALIGN = 64          # floats: the command rows start on a 256-byte boundary of the measurement buffer

    def _device_buffers(self, tick, dev):
        """the staging frame, the tables, the measurement buffer (``tick.static_in[1:]`` become two views of it: one upload) and
        the control, on ``dev``"""
        if self._frame_dev is not None and self._frame_dev.device == dev:
            return
        n_speed, n_cmd = tick.static_in[1].shape[1], tick.static_in[2].shape[1]
        if n_speed != 1:
            raise ValueError(f"AgentStep: the model's speed encoder takes {n_speed} numbers, the agent measures one")
        self.n_commands = n_cmd
        self._cmd_at = -(-self.B // self._ALIGN) * self._ALIGN
        i32 = torch.int32
        with torch.cuda.device(dev):
            self._frame_dev = torch.zeros(self.B, self.H0, self.W0, 4, dtype=torch.uint8, device=dev)
            self._htable, self._vtable = ((k, torch.tensor(b, dtype=i32, device=dev), torch.tensor(c, dtype=i32, device=dev))
                                          for k, b, c in (self._hcoeffs, self._vcoeffs))
            self._meas_dev = torch.zeros(self._cmd_at + self.B * n_cmd, dtype=torch.float32, device=dev)
            self._control_dev = torch.zeros(self.B, 3, dtype=torch.float64, device=dev)
        tick.static_in[1] = self._meas_dev[:self.B].view(self.B, 1)
        tick.static_in[2] = self._meas_dev[self._cmd_at:].view(self.B, n_cmd)

    @staticmethod
    def measurements(spd, cmd, batch, speed_factor, n_commands):
        """-> (speed f32 [B], one-hot command f32 [B, n_commands]) as ``image_agent.py:146-157`` builds them: the speed divided
        in double and rounded to f32 once; the command's index is ``cmd - 1``, or 3 when that is negative; an index the one-hot
        row does not have is a ``ValueError`` (the reference's ``scatter_`` fails there)."""
        speed = np.asarray(spd, dtype=np.float64).reshape(-1)
        command = np.asarray(cmd).reshape(-1)
        if speed.size != batch or command.size != batch:
            raise ValueError(f"AgentStep: {batch} speed(s) and command(s) expected, got {speed.size} and {command.size}")
        if command.dtype.kind not in "iu":
            raise TypeError("AgentStep: the command is the RoadOption's integer value")
        index = command.astype(np.int64) - 1
        index[index < 0] = 3
        if (index >= n_commands).any():
            raise ValueError(f"AgentStep: command {command.tolist()} has no place in a one-hot row of {n_commands}")
        onehot = np.zeros((batch, n_commands), dtype=np.float32)
        onehot[np.arange(batch), index] = 1.0
        return (speed / float(speed_factor)).astype(np.float32), onehot

    # ------------------------------------------------------------------ the tick's state
    last = property(lambda self: self.tick.last)
    draws_done = property(lambda self: self.tick.draws_done)

    def reset(self):
        self.tick.reset()

    def reseed(self, seed):
        self.tick.reseed(seed)

    # ------------------------------------------------------------------ one step
    def step(self, bgra, spd, cmd):
        if self.model.training:
            raise RuntimeError("AgentStep runs the eval-mode chain: call model.eval() first")
        shape = (self.B, self.H0, self.W0, 4)
        if not ((isinstance(bgra, np.ndarray) and bgra.dtype == np.uint8) or
                (isinstance(bgra, torch.Tensor) and bgra.dtype == torch.uint8 and not bgra.is_cuda)):
            raise TypeError("AgentStep: the frame is a uint8 numpy array or CPU tensor [H0,W0,4] (B, G, R, A)")
        if tuple(bgra.shape) != shape and not (self.B == 1 and tuple(bgra.shape) == shape[1:]):
            raise ValueError(f"AgentStep: the frame must be {shape[1:] if self.B == 1 else shape}, got {tuple(bgra.shape)}")
        speed, onehot = self.measurements(spd, cmd, self.B, self.speed_factor, self.n_commands)
        tick = self.tick
        tick._fresh()                            # (first: a model that moved takes the device buffers with it)
        if isinstance(bgra, torch.Tensor):
            self._frame_host.copy_(bgra.reshape(shape))
        else:
            np.copyto(self._frame_np, bgra.reshape(shape))
        self._meas_np[:self.B] = speed
        self._meas_np[self._cmd_at:] = onehot.reshape(-1)
        with torch.cuda.device(self._frame_dev.device):
            self._frame_dev.copy_(self._frame_host, non_blocking=True)
            self._meas_dev.copy_(self._meas_host, non_blocking=True)
            actions = tick._issue()
            if self.log is not None:             # (issued here, not recorded: the plan is the same with and without a log)
                self.log.push(tick.frames[:, -1], actions, tick.static_in[1], tick.static_in[2])
            self._control_host.copy_(self._control_dev, non_blocking=True)
            self._done.record()
        self._done.synchronize()
        return self._control_np.copy()
