"""The reference's `CorrespondenceModel` (cbctmc/registration/correspondence.py:29-226): a linear model that turns a breathing
signal into a displacement field, `field = mean + coefficients (signal - mean_signal)`, fitted by ordinary least squares
(Wilms et al. 2014, https://doi.org/10.1088/0031-9155/59/5/1147).  Same attributes, same pickle, same hash, so that files pass
between the two projects.  `build_default` produces the fields as the reference does: it registers every phase image of a 4D-CT
to the reference phase (`registration.register`, demons registration on the device: DESIGN.md row f14) and fits the model to the
result; `fit` takes fields and signals from anywhere.

The small part of `fit` (K x K or T x T matrices) runs on the host in float64 and follows the reference step by step.  The large
part is DEFINED by its order of operations, which the numpy route below and the device route (csrc/correspondence.hip) both
implement, so that they agree bit for bit:

    mean[v]           = float32((sum_t double(u_t[v])) / T)                       t = 0 .. T-1
    coefficients[v,k] = sum_t (double(u_t[v]) - double(mean[v])) * P[t,k]         t = 0 .. T-1, no fused multiply-add
    field32[v]        = float32(double(mean[v]) + (c[v,0] d[0] + c[v,1] d[1] + ...))   d = signal - mean_signal, left to right

With an engine context (`fit(..., ctx=ctx)`, `ctx.set_correspondence_model(model)`) the model is resident on the device and
`ctx.warp_geometry_by_signal(signal)` evaluates the field inside the warp kernel: a state change sends K doubles.
"""
from __future__ import annotations

import io
import pickle
from hashlib import sha256
from pathlib import Path

import numpy as np

PICKLE_KEYS = ("coefficients", "timesteps", "mean_signal", "signal_n_dims", "mean_vector_field", "spatial_shape", "signals", "reference_phase")
_CHUNK = 1 << 20  # elements per step of the host route (bounds the float64 temporaries)

# what a pickled model may name: the pieces numpy arrays and scalars are rebuilt from, and plain value types
_NUMPY_GLOBALS = {"_reconstruct", "ndarray", "dtype", "scalar", "_frombuffer"}
_NUMPY_MODULES = {"numpy", "numpy.core.multiarray", "numpy._core.multiarray", "numpy.core.numeric", "numpy._core.numeric"}
_BUILTIN_GLOBALS = {"tuple", "list", "dict", "set", "frozenset", "int", "float", "complex", "bool", "str", "bytes", "bytearray", "slice"}


class _ModelUnpickler(pickle.Unpickler):
    def find_class(self, module, name):
        if (module in _NUMPY_MODULES and name in _NUMPY_GLOBALS) or (module == "builtins" and name in _BUILTIN_GLOBALS) or \
                (module, name) == ("_codecs", "encode"):  # how protocol 2 carries an array's bytes
            return super().find_class(module, name)
        raise pickle.UnpicklingError(f"correspondence model file names {module}.{name}: only numpy arrays, numpy scalars and builtins are admitted")


class CorrespondenceModel:
    def __init__(self):
        self.coefficients = None        # float64 [3N, K]
        self.timesteps = None           # T
        self.mean_signal = None         # float64 [K, 1]
        self.signal_n_dims = None       # K
        self.mean_vector_field = None   # [3N, 1], dtype of the fields
        self.spatial_shape = None       # (x, y, z)
        self.signals = None             # [K, T]
        self.reference_phase = None
        self.inversion_reports = None   # of `inverted`: one report of registration.invert_field per training signal (not pickled)

    @property
    def is_fitted(self) -> bool:
        return all(v is not None for v in (self.coefficients, self.mean_signal, self.mean_vector_field))

    # -- files
    @property
    def model_hash(self) -> str:
        """SHA-256 over coefficients, timesteps (one byte), mean signal, mean field, signals, reference phase (one byte)."""
        if not self.is_fitted:
            raise RuntimeError("Correspondence model is not fitted")
        h = sha256()
        h.update(np.asarray(self.coefficients).tobytes())
        h.update(int(self.timesteps).to_bytes(1, "big"))
        h.update(np.asarray(self.mean_signal).tobytes())
        h.update(np.asarray(self.mean_vector_field).tobytes())
        h.update(np.asarray(self.signals).tobytes())
        h.update(int(self.reference_phase).to_bytes(1, "big"))
        return h.hexdigest()

    def save(self, filepath, include_model_hash: bool = True) -> Path:
        """Pickle of a plain dict with the reference's eight keys, as `<stem>[_<first 7 hex of the hash>].pkl`; returns the path."""
        filepath = Path(filepath).with_suffix(".pkl")
        if include_model_hash:
            filepath = filepath.with_name(f"{filepath.stem}_{self.model_hash[:7]}{filepath.suffix}")
        with open(filepath, "wb") as f:
            pickle.dump({key: getattr(self, key) for key in PICKLE_KEYS}, f)
        return filepath

    @classmethod
    def load(cls, filepath) -> "CorrespondenceModel":
        """A model saved here or by the reference.  The file may name numpy arrays, numpy scalars and builtins, nothing else."""
        with open(filepath, "rb") as f:
            data = _ModelUnpickler(io.BytesIO(f.read())).load()
        if not isinstance(data, dict) or not set(data) <= set(PICKLE_KEYS):
            raise pickle.UnpicklingError("not a correspondence model file: expected a dict of " + ", ".join(PICKLE_KEYS))
        model = cls()
        for key, value in data.items():
            setattr(model, key, value)
        return model

    # -- fit
    @staticmethod
    def _regularize_matrix(matrix: np.ndarray, condition_number_threshold: float = 30.0, step_size: float = 1e-3) -> np.ndarray:
        """Tikhonov steps on the diagonal until the condition number is at most the threshold (correspondence.py:97-147, step by
        step: a matrix of full rank and small condition number stays as it is; the loop gives up once the added value passes 1.0)."""
        added = 0.0
        condition_number = np.linalg.cond(matrix) if np.linalg.matrix_rank(matrix) == min(matrix.shape) else float("inf")
        while condition_number > condition_number_threshold:
            added += step_size
            condition_number = np.linalg.cond(matrix + np.eye(matrix.shape[0]) * added)
            if added > 1.0:
                raise RuntimeError("Abort matrix regularization. Tikhonov regularization reached 1.0.")
        return matrix + np.eye(matrix.shape[0]) * added

    @classmethod
    def signals_pseudo_inverse(cls, signals: np.ndarray):
        """The small part of `fit`: signals [T, K] -> (signals [K, T], mean_signal [K, 1], pseudo-inverse P [T, K] of the centred
        signals), through the covariance matrix of whichever side is smaller (correspondence.py:174-200)."""
        signals = np.asarray(signals, dtype=np.float64)
        timesteps = signals.shape[0]
        signals = signals.reshape(timesteps, -1).T
        n_dims = signals.shape[0]
        mean_signal = np.mean(signals, axis=1, keepdims=True)
        centered = signals - mean_signal
        if timesteps >= n_dims:
            covariance = cls._regularize_matrix(centered @ centered.T)   # K x K
            pinv = centered.T @ np.linalg.inv(covariance)
        else:
            covariance = cls._regularize_matrix(centered.T @ centered)   # T x T
            pinv = np.linalg.inv(covariance) @ centered.T
        return signals, mean_signal, np.ascontiguousarray(pinv)

    def fit(self, vector_fields: np.ndarray, signals: np.ndarray, reference_phase: int = 2, ctx=None, frame: str = "geometry"):
        """vector_fields [T, 3, x, y, z] (taken as float32), signals [T, K].  Without `ctx` the large part runs in numpy; with an
        engine context it runs on the device and leaves the model resident there (`frame` as for `Context.warp_geometry`);
        a model the device route does not take (K > 4, T > 64) is fitted on the host."""
        vector_fields = np.asarray(vector_fields, dtype=np.float32)
        if vector_fields.ndim != 5 or vector_fields.shape[1] != 3:
            raise ValueError(f"vector fields of shape {vector_fields.shape}, expected (timesteps, 3, x, y, z)")
        timesteps = vector_fields.shape[0]
        if np.shape(signals)[0] != timesteps:
            raise ValueError(f"{np.shape(signals)[0]} signals for {timesteps} vector fields")
        signals, mean_signal, pinv = self.signals_pseudo_inverse(signals)
        n_dims = signals.shape[0]
        mean = coefficients = None
        if ctx is not None:
            try:
                mean, coefficients = ctx.fit_correspondence_model(vector_fields, pinv, mean_signal, frame=frame)
            except RuntimeError as e:  # EngineError(-5): take the host route
                if getattr(e, "code", None) != -5:
                    raise
        on_device = mean is not None
        if not on_device:
            mean, coefficients = self._fit_fields_host(vector_fields.reshape(timesteps, -1), pinv)
        self.spatial_shape = tuple(vector_fields.shape[2:])
        self.timesteps = int(timesteps)
        self.signal_n_dims = int(n_dims)
        self.mean_signal = mean_signal
        self.mean_vector_field = mean.reshape(-1, 1)
        self.coefficients = coefficients
        self.signals = signals
        self.reference_phase = reference_phase
        if on_device:
            ctx._correspondence_model = self
        return self

    @staticmethod
    def _fit_fields_host(fields: np.ndarray, pinv: np.ndarray):
        """fields float32 [T, 3N], pinv [T, K] -> mean float32 [3N], coefficients float64 [3N, K]: the module's definition in numpy."""
        timesteps, n = fields.shape
        mean = np.empty(n, dtype=np.float32)
        coefficients = np.empty((n, pinv.shape[1]), dtype=np.float64)
        for a in range(0, n, _CHUNK):
            u = fields[:, a:a + _CHUNK].astype(np.float64)
            total = np.zeros(u.shape[1], dtype=np.float64)
            for t in range(timesteps):
                total = total + u[t]
            m = (total / np.float64(timesteps)).astype(np.float32)
            mean[a:a + _CHUNK] = m
            m64 = m.astype(np.float64)
            acc = np.zeros((u.shape[1], pinv.shape[1]), dtype=np.float64)
            for t in range(timesteps):
                centred = u[t] - m64
                for k in range(pinv.shape[1]):
                    acc[:, k] = acc[:, k] + centred * pinv[t, k]
            coefficients[a:a + _CHUNK] = acc
        return mean, coefficients

    # -- build
    @classmethod
    def build_default(cls, images, signals=None, masks=None, timepoints=None, reference_phase: int = 2, masked_registration: bool = True, ctx=None,
                      gpu_id: int = 0, inverse: bool = False, **register_parameters) -> "CorrespondenceModel":
        """The reference's `build_default` (correspondence.py:277-356): images [T, x, y, z] of a 4D-CT (arrays as an MCGeometry holds
        them) -> a fitted model.

        signals [T, K] as `fit` takes them, or None: then amplitude and rate of change come from `masks` [T, x, y, z] (lung masks)
        and `timepoints` [T] through `RespiratorySignal.from_masks`, interpolated at the timepoints, one (amplitude, rate) row per
        phase.  (The reference stacks the two curves as [2, T] and leaves it to the reshape(T, -1) in its `fit` to make rows of them,
        which pairs values of different phases; that is not repeated here.)  Every phase t, the reference phase included (its field is exactly zero), is registered with
        moving = images[reference_phase] and fixed = images[t], so that field t takes the reference phase to phase t: what `fit`,
        `MCGeometry.warp` and the engine's warp expect.  With masked_registration and masks, masks[t] is the fixed mask; the moving
        mask of the reference's call has no counterpart in the rule of row f14 and is not used.  There is no affine stage.
        register_parameters go to `registration.register` (iterations, tau, sigma, n_levels; the reference's values are the
        defaults).  With an engine context the fit runs on the device and leaves the model resident there.  The lung segmentation
        shortcut of the reference (`_segment_lungs`, which loads a network from a fixed path) is not part of this package: masks are
        inputs.

        DIRECTION.  The default (inverse=False) gives pull-back fields: phase_t(x) ~ ref(x + u_t(x)), field t says where in the
        reference phase the content of phase t's voxel x comes from -- what the warps of the simulation consume.  inverse=True
        registers every phase t with moving = images[t] and fixed = images[reference_phase] (fixed mask: masks[reference_phase]),
        so that ref(x) ~ phase_t(x + u_t(x)): the fitted model then takes a voxel of the reference phase to the position of its
        material at a state, which is what `reconstruction.MotionModel.from_correspondence_model` (motion-compensated FDK)
        expects.  The two are different models; here neither is derived from the other, and a pull-back model handed to the
        reconstruction is NOT silently inverted.  `build_pair` gives both from one sweep: it derives the second from the first by
        field inversion (`inverted`), which also makes the two consistent with each other."""
        from . import registration
        from .respiratory import RespiratorySignal
        if signals is None:
            if masks is None:
                raise ValueError("Either signals or masks must be given")
            if timepoints is None:
                raise ValueError("timepoints must be given if masks are given")
            respiratory_signal = RespiratorySignal.from_masks(masks=masks, timepoints=timepoints)
            signal = np.interp(timepoints, respiratory_signal.time, respiratory_signal.signal)
            dt_signal = np.interp(timepoints, respiratory_signal.time, respiratory_signal.dt_signal)
            signals = np.stack([signal, dt_signal], axis=1)
        timesteps = len(images)
        if not 0 <= int(reference_phase) < timesteps:
            raise ValueError(f"reference_phase {reference_phase} is outside the {timesteps} images")
        if masks is not None and len(masks) != timesteps:
            raise ValueError(f"{len(masks)} masks for {timesteps} images")
        if np.shape(signals)[0] != timesteps:
            raise ValueError(f"{np.shape(signals)[0]} signals for {timesteps} images")
        reference = images[int(reference_phase)]
        vector_fields = []
        for t in range(timesteps):
            if inverse:
                fixed_mask = masks[int(reference_phase)] if masked_registration and masks is not None else None
                field, _ = registration.register(reference, images[t], fixed_mask=fixed_mask, gpu_id=gpu_id, **register_parameters)
            else:
                fixed_mask = masks[t] if masked_registration and masks is not None else None
                field, _ = registration.register(images[t], reference, fixed_mask=fixed_mask, gpu_id=gpu_id, **register_parameters)
            vector_fields.append(field)
        return cls().fit(np.stack(vector_fields, axis=0), signals, reference_phase=reference_phase, ctx=ctx)

    # -- the opposite direction
    def inverted(self, iterations: int = 40, relaxation: float = 0.5, tolerance: float = 0.05, ctx=None, gpu_id: int = 0, _invert=None) -> "CorrespondenceModel":
        """The model of the opposite direction, derived from this one without a second registration sweep: for
        every training signal t the field this model PREDICTS, `predict_field32(signals[t])`, is inverted on the device
        (`registration.invert_field`: v with u(x + v(x)) + v(x) ~ 0) and a new model is fitted to the inverses with the same
        signals and reference phase (`fit(..., ctx=ctx)`: with an engine context on the device, which then holds the NEW model).
        The new model carries `inversion_reports`, one report of `invert_field` per training signal; RuntimeError if one of them ends
        with a max residual above `tolerance` voxels (a predicted field that folds has no inverse), or if this model is not fitted.

        What the result is and is not.  It is the linear fit to the inverses of the fields that this model predicts at its training
        signals.  The inverse of a linear model is not linear in the signal, so the two models are not exact inverses of each other
        between or even at those signals: the pair's residual (`pair_residual`) is of second order, not zero -- 0.05 to 0.12 voxel rms
        on the test fixture (a sphere moved by 2 voxels per unit amplitude), against 0.25 to 1.07 for two independently registered
        models.  These are float64 numbers of the restatement on that fixture; nothing has been measured on a clinical field.
        `_invert` replaces `registration.invert_field` (tests pass the restatement: the plumbing runs without a GPU)."""
        from . import registration
        if not self.is_fitted:
            raise RuntimeError("Correspondence model is not fitted")
        invert = registration.invert_field if _invert is None else _invert
        signals = np.asarray(self.signals, dtype=np.float64)  # [K, T]
        fields, reports = [], []
        for t in range(signals.shape[1]):
            inverse, report = invert(self.predict_field32(signals[:, t]), iterations=iterations, relaxation=relaxation, gpu_id=gpu_id)
            registration.check_residual(report, tolerance)
            fields.append(np.asarray(inverse, dtype=np.float32))
            reports.append(report)
        model = type(self)().fit(np.stack(fields, axis=0), signals.T, reference_phase=self.reference_phase, ctx=ctx)
        model.inversion_reports = reports
        return model

    @classmethod
    def build_pair(cls, images, signals=None, masks=None, timepoints=None, reference_phase: int = 2, masked_registration: bool = True, ctx=None, gpu_id: int = 0,
                   inversion: dict = None, **register_parameters):
        """-> (from_reference, to_reference): both directions from ONE registration sweep, the recommended way to obtain them.
        from_reference = `build_default(images, ...)` (pull-back fields: what the warps of the simulation consume; with `ctx` it is
        fitted on the device and stays resident there); to_reference = `from_reference.inverted(**inversion)` (what
        `reconstruction.MotionModel.from_correspondence_model` expects; fitted on the host, so that the context keeps
        from_reference).  `inversion`: iterations, relaxation, tolerance of `inverted`; register_parameters go to
        `registration.register` as in `build_default`.  The pair is consistent to second order, not exactly (`inverted`)."""
        if "inverse" in register_parameters:
            raise ValueError("build_pair fixes the directions itself: `inverse` belongs to build_default")
        from_reference = cls.build_default(images, signals=signals, masks=masks, timepoints=timepoints, reference_phase=reference_phase,
                                           masked_registration=masked_registration, ctx=ctx, gpu_id=gpu_id, **register_parameters)
        return from_reference, from_reference.inverted(gpu_id=gpu_id, **(inversion or {}))

    def pair_residual(self, other: "CorrespondenceModel", signal, gpu_id: int = 0) -> dict:
        """{"max", "rms"} in voxels of r(x) = v(x) + u(x + v(x)), u = this model's and v = the other's `predict_field32(signal)`
        (`registration.composition_residual`): how far the two are from being each other's inverse at that signal.  Two models of
        the SAME direction give about 2 |u| (5.2 voxel rms at an end state of the test fixture): that mistake is detected.  A pair
        handed over in the wrong order is not: swapping the arguments leaves the residual small (it changes only where the clamp at
        the border acts: 0.10 to 0.67 voxel rms on the fixture, less than two independently registered models give).  ValueError
        where the spatial shapes or `signal_n_dims` differ."""
        from . import registration
        if not (self.is_fitted and other.is_fitted):
            raise RuntimeError("Correspondence model is not fitted")
        if tuple(self.spatial_shape) != tuple(other.spatial_shape) or int(self.signal_n_dims) != int(other.signal_n_dims):
            raise ValueError(f"models of spatial shapes {tuple(self.spatial_shape)} and {tuple(other.spatial_shape)} with {self.signal_n_dims} and "
                             f"{other.signal_n_dims} signal dimensions do not form a pair")
        _, report = registration.composition_residual(self.predict_field32(signal), other.predict_field32(signal), gpu_id=gpu_id)
        return {"max": report["residual_max"], "rms": report["residual_rms"]}

    # -- predict
    def _predict64(self, signal: np.ndarray) -> np.ndarray:
        if not self.is_fitted:
            raise RuntimeError("Correspondence model is not fitted")
        signal = np.asarray(signal)
        if signal.shape != (self.signal_n_dims,):
            raise ValueError(f"Given signal has wrong shape. Expected ({self.signal_n_dims},), but got {signal.shape}")
        d = signal.astype(np.float64) - np.asarray(self.mean_signal, dtype=np.float64).reshape(-1)
        mean = np.asarray(self.mean_vector_field).reshape(-1)
        coefficients = np.asarray(self.coefficients)
        out = np.empty(mean.shape[0], dtype=np.float64)
        for a in range(0, mean.shape[0], _CHUNK):
            c = coefficients[a:a + _CHUNK].astype(np.float64, copy=False)
            acc = c[:, 0] * d[0]
            for k in range(1, d.shape[0]):
                acc = acc + c[:, k] * d[k]
            out[a:a + _CHUNK] = mean[a:a + _CHUNK].astype(np.float64) + acc
        return out

    def predict(self, signal: np.ndarray) -> np.ndarray:
        """float64 [3, x, y, z] like the reference's `predict`: the value the engine's field is the float32 rounding of."""
        return self._predict64(signal).reshape(3, *self.spatial_shape)

    def predict_field32(self, signal: np.ndarray) -> np.ndarray:
        """float32 [3, x, y, z]: the field the engine consumes (and evaluates itself from a resident model), bit for bit."""
        return self._predict64(signal).astype(np.float32).reshape(3, *self.spatial_shape)
