"""Training of the speed-up network without a GPU (4d-cbct-mc_amd/speedup_training.py, csrc/speedup_train.hip): the numpy
statements of the rule (speedup_train_ref.py) against torch's losses, optimiser and autograd, the initialisation, the files the
trainer writes, the dataset, every refusal of the C ABI on a planned (dry) handle, and the fact the zero bias gradients rest on."""
import ctypes as C
import json
import logging

import numpy as np
import pytest

import cases
import speedup_ref
import speedup_train_ref as ref

torch = pytest.importorskip("torch")
import torch.nn.functional as F  # noqa: E402

speedup = cases.pkg.speedup
training = cases.pkg.speedup_training
recon = cases.pkg.reconstruction

SMALL = dict(mean_net=(2, 1, 4), var_net=(1, 1, 4))


def _t(a, grad=False):
    t = torch.as_tensor(np.asarray(a, dtype=np.float64))
    return t.clone().requires_grad_(True) if grad else t


# ------------------------------------------------------------------------------------------------------------------ the rule
def test_loss_statements_equal_torch_with_autograd():
    """Both losses and their gradients into the nets' outputs, to 1e-12, with a pixel whose variance lies under the clamp, a pixel
    whose mean is clipped by the relu and a pixel with m == t."""
    rng = np.random.default_rng(0)
    lp = rng.uniform(1.0, 4.0, size=(2, 6, 8))
    net = rng.normal(0.0, 0.05, size=lp.shape)
    lp[0, 0, 0], net[0, 0, 0] = 0.2, -0.5  # lp + 10 tanh(net) < 0: clipped
    net_t = _t(net, grad=True)
    m_t = torch.relu(_t(lp) + 10.0 * torch.tanh(net_t))
    t = m_t.detach().numpy() + rng.choice([-1.0, 1.0], size=lp.shape) * rng.uniform(0.2, 0.5, size=lp.shape)
    t[1, 2, 3] = m_t.detach().numpy()[1, 2, 3]  # m == t: sign 0
    want = F.l1_loss(m_t, _t(t))
    want.backward()
    loss, dl_dm = ref.l1_loss(m_t.detach().numpy(), t)
    assert abs(loss - float(want.detach())) <= 1e-12
    got = ref.head_mean_grad(lp, net, dl_dm)
    assert got[0, 0, 0] == 0.0 and got[1, 2, 3] == 0.0 and np.count_nonzero(got) == got.size - 2
    assert np.abs(got - net_t.grad.numpy()).max() <= 1e-12

    m = m_t.detach().numpy()
    s = rng.normal(0.0, 1.0, size=lp.shape)
    s_t = _t(s, grad=True)
    v_t = _t(m) * (0.10 * torch.sigmoid(s_t)) + 1e-6
    assert float(v_t.detach()[0, 0, 0]) == 1e-6  # m = 0 there: v is the floor itself, not above it
    want = F.gaussian_nll_loss(_t(m), _t(t), v_t)
    want.backward()
    loss, dl_dv = ref.nll_loss(m, v_t.detach().numpy(), t)
    assert abs(loss - float(want.detach())) <= 1e-12 * max(1.0, abs(float(want.detach())))
    got = ref.head_variance_grad(m, s, dl_dv)
    assert got[0, 0, 0] == 0.0
    scale = np.abs(s_t.grad.numpy()).max()
    assert np.abs(got - s_t.grad.numpy()).max() <= 1e-12 * max(1.0, scale)
    # A variance given below the clamp, which the head cannot produce (v >= 1e-6, with equality only where m = 0 and dv/ds = 0):
    # the loss is torch's; the rule gives no gradient there, while torch clamps outside the graph and lets the clamped pixel's
    # gradient 0.5 (1 / eps - d^2 / eps^2) / N through.  Everywhere else the two gradients are equal.
    v = v_t.detach().numpy().copy()
    v[1, 1, 1] = 1e-7
    v_in = _t(v, grad=True)
    want = F.gaussian_nll_loss(_t(m), _t(t), v_in)
    want.backward()
    loss, dl_dv = ref.nll_loss(m, v, t)
    assert abs(loss - float(want.detach())) <= 1e-12 * max(1.0, abs(float(want.detach())))
    assert dl_dv[1, 1, 1] == 0.0
    d = m[1, 1, 1] - t[1, 1, 1]
    assert abs(float(v_in.grad[1, 1, 1]) / (0.5 * (1e6 - d * d * 1e12) / m.size) - 1.0) <= 1e-12
    rest = v > 1e-6  # all but that pixel and the one at the floor itself (m = 0), where dL/dv is not passed on: dv/ds = 0 there
    assert rest.size - np.count_nonzero(rest) == 2 and dl_dv[0, 0, 0] == 0.0
    assert np.abs(dl_dv - v_in.grad.numpy())[rest].max() <= 1e-12 * np.abs(dl_dv).max()


def test_adam_statements_equal_torch_over_five_steps():
    rng = np.random.default_rng(1)
    w0 = rng.normal(size=50)
    grads = [rng.normal(size=50) * 10.0 ** rng.integers(-6, 2) for _ in range(5)]
    p = _t(w0, grad=True)
    opt = torch.optim.Adam([p], lr=1e-3)
    sched = torch.optim.lr_scheduler.ExponentialLR(opt, gamma=0.99999)
    w, m, v, lr = w0, np.zeros(50), np.zeros(50), 1e-3
    w2, m2, v2 = w0, np.zeros(50), np.zeros(50)
    for t, g in enumerate(grads, start=1):
        p.grad = _t(g)
        opt.step()
        sched.step()
        w, m, v = ref.adam(w, g, m, v, t, lr)
        w2, m2, v2 = training.adam_step(w2, g, m2, v2, t, lr)
        lr *= 0.99999
        assert np.abs(w - p.detach().numpy()).max() <= 1e-12
        assert np.abs(w2 - p.detach().numpy()).max() <= 1e-12
    assert np.abs(m - opt.state[p]["exp_avg"].numpy()).max() <= 1e-12 and np.abs(v - opt.state[p]["exp_avg_sq"].numpy()).max() <= 1e-12
    w3, m3, v3 = ref.adam(w0, np.zeros(50), np.zeros(50), np.zeros(50), 1, 1e-3)  # no gradient, no moments: nothing moves
    assert np.array_equal(w3, w0) and not m3.any() and not v3.any()


@pytest.mark.parametrize("shape", [(1, 1), (2, 2), (5, 7)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("sources", [(3, 0), (2, 3)], ids=["one", "skip+upsampled"])
def test_input_gradient_statement_equals_autograd(shape, sources):
    """Extended correlation + fold, split into the two sources, against autograd of conv3x3 on cat([a, upsample(b)]), to 1e-12."""
    H, W = shape
    c1, c2 = sources
    rng = np.random.default_rng(H * 10 + W + c2)
    a = _t(rng.normal(size=(1, c1, H, W)), grad=True)
    b = _t(rng.normal(size=(1, c2, (H + 1) // 2, (W + 1) // 2)), grad=True) if c2 else None
    w = rng.normal(size=(4, c1 + c2, 3, 3))
    dy = rng.normal(size=(4, H, W))
    x = a if b is None else torch.cat([a, F.interpolate(b, scale_factor=2, mode="nearest")[:, :, :H, :W]], dim=1)
    speedup_ref.conv3x3(x, _t(w), _t(np.zeros(4))).backward(_t(dy)[None])
    g1, g2 = ref.conv_dgrad(dy, w, c1, upsample=bool(c2))
    assert np.abs(g1 - a.grad[0].numpy()).max() <= 1e-12
    if c2:
        assert g2.shape == b.shape[1:] and np.abs(g2 - b.grad[0].numpy()).max() <= 1e-12
    else:
        assert g2 is None


def test_weight_gradient_statement_equals_autograd():
    rng = np.random.default_rng(4)
    x = rng.normal(size=(3, 5, 7))
    dy = rng.normal(size=(4, 5, 7))
    w, b = _t(rng.normal(size=(4, 3, 3, 3)), grad=True), _t(np.zeros(4), grad=True)
    speedup_ref.conv3x3(_t(x)[None], w, b).backward(_t(dy)[None])
    dw, db = ref.conv_wgrad(x, dy)
    assert np.abs(dw - w.grad.numpy()).max() <= 1e-12 and np.abs(db - b.grad.numpy()).max() <= 1e-12


def test_maxpool_rule_on_windows_with_ties():
    """The first maximum in the order (0,0), (0,1), (1,0), (1,1) takes the gradient: torch's rule."""
    x = np.array([[[1, 1, 5, 2, 0, 0], [1, 1, 2, 5, 0, 7], [3, 4, 9, 9, -1, -1], [4, 3, 9, 9, -1, -2]]], dtype=np.float64)
    dy = np.arange(1, 7, dtype=np.float64).reshape(1, 2, 3)
    want = np.zeros_like(x)
    for (y, xx), v in zip([(0, 0), (0, 2), (1, 5), (2, 1), (2, 2), (2, 4)], dy.ravel()):
        want[0, y, xx] = v
    assert np.array_equal(ref.maxpool_backward(x, dy), want)
    t = _t(x, grad=True)
    F.max_pool2d(t[None], 2).backward(_t(dy)[None])
    assert np.array_equal(t.grad.numpy(), want)
    odd = np.random.default_rng(2).integers(0, 3, size=(2, 5, 7)).astype(np.float64)  # many ties, an odd last row and column
    g = np.random.default_rng(3).normal(size=(2, 2, 3))
    t = _t(odd, grad=True)
    F.max_pool2d(t[None], 2).backward(_t(g)[None])
    assert np.array_equal(ref.maxpool_backward(odd, g), t.grad.numpy())


def test_norm_backward_statement_equals_autograd():
    rng = np.random.default_rng(5)
    x, dy = rng.normal(1.0, 2.0, size=(3, 6, 10)), rng.normal(size=(3, 6, 10))
    got, want = ref.norm_lrelu_backward_statement(x, dy), ref.norm_lrelu_backward(x, dy)
    assert np.abs(got - want).max() <= 1e-12
    assert np.abs(want.sum(axis=(1, 2))).max() <= 1e-12


def test_bias_gradient_of_a_normed_convolution_is_zero_in_float64():
    """What the deviation rests on: in float64 autograd the gradient of every bias that feeds an instance norm is below 1e-12 x the
    largest weight gradient, in both phases."""
    tensors = speedup.state_dict_tensors((2, 2, 8), (1, 2, 8))
    weights = speedup_ref.seeded_weights(7, tensors)
    lp, fp = speedup_ref.seeded_inputs(7, 2, 16, 24)
    m64, _ = speedup_ref.predict(weights, lp, fp)
    t = (m64 + 0.3).astype(np.float32)
    for phase, net in (("mean", "mean_net"), ("variance", "var_net")):
        _, grads = ref.loss_and_gradients(weights, lp, fp, t, phase)
        largest = max(np.abs(g).max() for n, g in grads.items() if n.startswith(net) and n.endswith(".weight"))
        assert largest > 0
        normed = [n for n in ref.normed_biases(grads) if n.startswith(net)]
        assert len(normed) == 8
        for n in normed:
            assert np.abs(grads[n]).max() <= 1e-12 * largest, n
        other = "var_net" if net == "mean_net" else "mean_net"
        assert all(not g.any() for n, g in grads.items() if n.startswith(other))


# ------------------------------------------------------------------------------------------------- initialisation and files
def test_initialisation_is_uniform_within_the_bound_of_a_default_convolution():
    w = training.initial_weights(3)
    assert [(n, v.shape) for n, v in w.items()] == speedup.state_dict_tensors()
    for name, shape in speedup.state_dict_tensors():
        c_in = shape[1] if name.endswith(".weight") else w[name[:-4] + "weight"].shape[1]
        bound = 1.0 / np.sqrt(9.0 * c_in)
        assert w[name].dtype == np.float32 and np.abs(w[name]).max() <= np.float32(bound), name
        if w[name].size >= 4096:  # the uniform distribution fills the interval: sd = bound / sqrt(3)
            assert np.abs(w[name]).max() > 0.99 * bound and abs(w[name].std() * np.sqrt(3.0) / bound - 1.0) < 0.05, name
    again, other = training.initial_weights(3), training.initial_weights(4)
    assert all(np.array_equal(w[k], again[k]) for k in w) and not np.array_equal(w["mean_net.init_conv.weight"], other["mean_net.init_conv.weight"])


def test_state_dict_and_saved_files_round_trip_through_the_loader(tmp_path):
    trainer = training.MCSpeedupTrainer(seed=5)
    state = trainer.state_dict()
    golden = [(n, tuple(s)) for n, s in json.loads((speedup_ref.GOLDEN / "speedup_state_dict.json").read_text())]
    assert [(n, v.shape) for n, v in state.items()] == [g for g in golden if g[0] != "var_scale"] + [g for g in golden if g[0] == "var_scale"]
    assert sorted(state) == sorted(n for n, _ in golden)
    assert state["var_scale"].dtype == np.float32 and state["var_scale"][0] == np.float32(0.001)
    want = np.concatenate([state[n].ravel() for n, _ in speedup.state_dict_tensors()])
    for suffix in (".npz", ".pth"):
        path = trainer.save(tmp_path / "models" / ("step_0" + suffix))
        model = speedup.MCSpeedup.from_filepath(path)
        assert model.mean_net == (2, 4, 64) and model.var_net == (1, 2, 16) and np.array_equal(model.flat, want)
    assert set(torch.load(tmp_path / "models" / "step_0.pth")) == {"model"}
    with pytest.raises(ValueError, match="npz or .pth"):
        trainer.save(tmp_path / "weights.bin")
    small = training.MCSpeedupTrainer(weights=speedup_ref.seeded_weights(2, speedup.state_dict_tensors(**SMALL)), **SMALL)
    check = small.save_checkpoint(tmp_path / "check.npz")
    other = training.MCSpeedupTrainer(seed=1, **SMALL)
    other.load_checkpoint(check)
    assert np.array_equal(other._flat, small._flat) and other.i_step == 0 and other._lr == 1e-3
    with pytest.raises(ValueError, match="architecture"):
        trainer.load_checkpoint(check)
    with pytest.raises(ValueError, match="joint stage"):
        training.MCSpeedupTrainer(n_pretrain_steps=None, **SMALL)
    phases = training.MCSpeedupTrainer(n_pretrain_steps=2, **SMALL)
    assert phases.phase == "mean"
    phases.i_step = 2
    assert phases.phase == "variance"


def test_dataset_finds_complete_triples_and_skips_the_rest(tmp_path, caplog):
    rng = np.random.default_rng(0)
    name = lambda pat, kind, proj, phase=0: tmp_path / f"pat_{pat:03d}__phase_{phase:02d}__{kind}__proj_{proj:03d}.npy"  # noqa: E731
    for pat in (22, 104):
        for proj in range(3):
            for kind in ("speedup_20.00x", "fp", "reference"):
                np.save(name(pat, kind, proj), rng.normal(size=(4, 6)))
    np.save(name(22, "speedup_50.00x", 0), np.ones((4, 6)))
    name(104, "fp", 2).unlink()
    assert training.MCSpeedUpDataset.get_patient_ids_from_folder(tmp_path) == [22, 104]
    with caplog.at_level(logging.WARNING):
        ds = training.MCSpeedUpDataset.from_folder(tmp_path, modes=["speedup_20.00x", "speedup_50.00x"], patient_ids=[22, 104], projections=range(5))
    assert [(e["patient_id"], e["mode"], e["projection"]) for e in ds.filepaths] == \
        [(22, "speedup_20.00x", 0), (22, "speedup_20.00x", 1), (22, "speedup_20.00x", 2), (22, "speedup_50.00x", 0), (104, "speedup_20.00x", 0),
         (104, "speedup_20.00x", 1)]
    assert "pat_104__phase_00__speedup_20.00x__proj_002.npy" in caplog.text
    item = ds[3]
    assert item["low_photon"].shape == (1, 4, 6) and item["low_photon"].dtype == np.float32 and np.all(item["low_photon"] == 1) and item["mode"] == "speedup_50.00x"
    assert np.array_equal(item["high_photon"][0], np.load(name(22, "reference", 0)).astype(np.float32))
    assert len(ds[1:3]) == 2 and len(ds[np.array([0, 5])]) == 2
    batch = ds.batch([0, 4])
    assert batch["low_photon"].shape == (2, 1, 4, 6) and batch["patient_id"] == [22, 104]


def test_write_speedup_dataset_cuts_the_scan_outputs_into_the_layout(tmp_path):
    rng = np.random.default_rng(1)
    low, high, fp = (rng.normal(size=(3, 4, 6)).astype(np.float32) for _ in range(3))
    for config, stack in (("speedup_20.00x", low), ("reference", high)):
        (tmp_path / "sim" / config).mkdir(parents=True)
        recon.write_mha(tmp_path / "sim" / config / "projections_total_normalized.mha", stack, [1.0, 1.0, 1.0], [0.0, 0.0, 0.0])
    recon.write_mha(tmp_path / "sim" / "density_fp.mha", fp, [1.0, 1.0, 1.0], [0.0, 0.0, 0.0])
    assert training.write_speedup_dataset(tmp_path / "sim", "speedup_20.00x", "reference", tmp_path / "data", patient_id=7, phase=2) == 3
    ds = training.MCSpeedUpDataset.from_folder(tmp_path / "data", modes=["speedup_20.00x"], patient_ids=[7], phases=(2,), projections=range(3))
    assert len(ds) == 3
    batch = ds.batch(range(3))
    assert np.array_equal(batch["low_photon"][:, 0], low) and np.array_equal(batch["high_photon"][:, 0], high) and np.array_equal(batch["forward_projection"][:, 0], fp)


# ----------------------------------------------------------------------------------------------------- refusals of the C ABI
def _options(flat, nu=32, nv=32, max_batch=2, mean=(2, 2, 4), var=(1, 1, 4), dry=1, lr=1e-3, gamma=0.99999, n_weights=None):
    return training._TrainOptions(C.sizeof(training._TrainOptions), 0, nu, nv, max_batch, *mean, *var, dry, flat.ctypes.data if flat is not None else None,
                                  flat.size if n_weights is None else n_weights, lr, gamma, 0.9, 0.999)


def test_abi_refusals_come_before_any_device_call(engine):
    """A planned (dry) handle touches no device: every refusal of a batch is reached on it, and only then the refusal to run."""
    lib = training._library()
    n = sum(int(np.prod(s)) for _, s in speedup.state_dict_tensors((2, 2, 4), (1, 1, 4)))
    flat = np.zeros(n, np.float32)
    handle = C.c_void_p()

    def create_refused(o, text):
        h = C.c_void_p()
        assert lib.mcgpu_speedup_train_create(C.byref(o) if o is not None else None, C.byref(h)) == -1 and not h.value
        assert text in lib.mcgpu_last_error().decode(), lib.mcgpu_last_error().decode()

    create_refused(None, "struct_size")
    create_refused(_options(None, n_weights=n), "weights is NULL")
    create_refused(_options(flat, n_weights=n - 1), f"n_weights is {n - 1} but the architecture has {n} values")
    create_refused(_options(flat, nu=34), "must be divisible by 4 (2^levels)")
    create_refused(_options(flat, nv=30), "must be divisible by 4 (2^levels)")
    create_refused(_options(flat, nu=4, nv=4), "fewer than 2 pixels")
    create_refused(_options(flat, max_batch=0), "max_batch must be >= 1")
    create_refused(_options(flat, mean=(3, 2, 4)), "bad architecture")
    create_refused(_options(flat, lr=0.0), "lr must be > 0")
    create_refused(_options(flat, gamma=1.5), "gamma in (0, 1]")
    assert lib.mcgpu_speedup_train_create(C.byref(_options(flat)), None) == -1

    assert lib.mcgpu_speedup_train_create(C.byref(_options(flat)), C.byref(handle)) == 0 and handle.value
    lp, fp = speedup_ref.seeded_inputs(1, 2, 32, 32)
    t = lp + np.float32(0.3)
    rep = training._TrainReport(struct_size=C.sizeof(training._TrainReport))
    ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731

    def refused(text, h=handle, phase=0, n=2, a=lp, b=fp, c=t, report=rep, gradients=False):
        if gradients:
            rc = lib.mcgpu_speedup_train_gradients(h, phase, n, ptr(a), ptr(b), ptr(c), None, C.byref(report))
        else:
            rc = lib.mcgpu_speedup_train_step(h, phase, n, ptr(a), ptr(b), ptr(c), 1, C.byref(report) if report is not None else None)
        assert rc == -1
        assert text in lib.mcgpu_last_error().decode(), lib.mcgpu_last_error().decode()

    refused("handle is NULL", h=None)
    refused("unknown phase 2", phase=2)
    refused("unknown phase -1", phase=-1)
    refused("n is 3 but the trainer was created for 1..2", n=3)
    refused("n is 0 but", n=0)
    refused("low_photon is NULL", a=None)
    refused("high_photon is NULL", c=None)
    refused("forward_projection is NULL", b=None)
    flat_fp = fp.copy()
    flat_fp[1] = 2.5
    refused("forward_projection slice 1 has zero variance", b=flat_fp)
    refused("report->struct_size", report=training._TrainReport(struct_size=4))
    refused("flat_gradient is NULL", gradients=True)
    refused("dry plan")  # everything in order: only now the handle says that it cannot run
    assert lib.mcgpu_speedup_train_predict(handle, 2, ptr(lp), None, None, None) == -1 and "forward_projection is NULL" in lib.mcgpu_last_error().decode()
    state = training._TrainState(struct_size=C.sizeof(training._TrainState))
    assert lib.mcgpu_speedup_train_get_state(handle, C.byref(state)) == 0
    assert state.n_weights == n and state.step_mean == 0 and state.lr == 1e-3
    # the weights, two moments and the gradient, and two sets of activations of a 32 x 32 sample
    assert 4 * 4 * n + 32 * 32 * 4 * 20 < state.planned_device_bytes < 64 * 2 ** 20
    state.weights, state.n_weights = flat.ctypes.data, n - 1
    assert lib.mcgpu_speedup_train_get_state(handle, C.byref(state)) == -1 and f"the trainer has {n} values" in lib.mcgpu_last_error().decode()
    assert lib.mcgpu_speedup_train_set_state(handle, C.byref(state)) == -1
    assert lib.mcgpu_speedup_train_get_state(handle, None) == -1 and "mcgpu_speedup_train_state" in lib.mcgpu_last_error().decode()
    assert lib.mcgpu_speedup_train_destroy(handle) == 0 and lib.mcgpu_speedup_train_destroy(None) == 0

    one = sum(int(np.prod(s)) for _, s in speedup.state_dict_tensors((1, 2, 4), (1, 1, 4)))
    assert lib.mcgpu_speedup_train_create(C.byref(_options(np.zeros(one, np.float32), mean=(1, 2, 4))), C.byref(handle)) == 0
    refused("forward_projection must be NULL", h=handle)
    lib.mcgpu_speedup_train_destroy(handle)


def test_planned_device_bytes_of_the_python_trainer(engine):
    small = training.MCSpeedupTrainer(seed=1, **SMALL)
    a, b = small.planned_device_bytes(1, 32, 48), small.planned_device_bytes(1, 64, 96)
    assert 0 < a < b


def test_stage_refusals_come_before_any_device_call(engine):
    lib = training._library()
    buf = np.zeros(64, np.float32)
    values = np.zeros(4)
    p = buf.ctypes.data

    def args(**kw):
        return training._TrainStageArgs(struct_size=C.sizeof(training._TrainStageArgs), **kw)

    for stage, a, text in [(9, args(nu=4, nv=4, in_=p, out=p, c1=1), "unknown stage 9"),
                           (0, args(nu=4, nv=4, in_=p, c1=1), "in or out is NULL"),
                           (2, args(nu=4, nv=4, in_=p, out=p, c1=1), "in2 is NULL"),
                           (0, args(nu=4, nv=4, in_=p, out=p, c1=1, c_out=1), "in2 or in3 is NULL"),
                           (0, args(nu=4, nv=4, in_=p, out=p, in3=p, c1=1, c2=1, c_out=1), "in2 or in3 is NULL"),
                           (1, args(nu=4, nv=4, in_=p, in2=p, out=p, c1=1, c2=1, c_out=1), "out2 is NULL"),
                           (3, args(nu=4, nv=4, in_=p, in2=p, out=p, c1=0), "c1 must be"),
                           (2, args(nu=1, nv=1, in_=p, in2=p, out=p, c1=1), "at least 2 pixels"),
                           (4, args(nu=4, nv=4, in_=p, in2=p, out=p, n=1), "in3 or values is NULL"),
                           (5, args(nu=4, nv=4, in_=p, in2=p, in3=p, out=p, values=values.ctypes.data, n=0), "n is 0"),
                           (6, args(in_=p, out=p, out2=p, n=4, step=1, beta1=0.9, beta2=0.999), "out2 or out3 is NULL"),
                           (6, args(in_=p, out=p, out2=p, out3=p, n=4, step=0, beta1=0.9, beta2=0.999), "step is 0"),
                           (6, args(in_=p, out=p, out2=p, out3=p, n=4, step=1, beta1=1.0, beta2=0.999), "beta1 and beta2")]:
        assert lib.mcgpu_speedup_train_stage(stage, C.byref(a), None) == -1
        assert text in lib.mcgpu_last_error().decode(), (stage, lib.mcgpu_last_error().decode())
    assert lib.mcgpu_speedup_train_stage(0, None, None) == -1
    assert "mcgpu_speedup_train_stage_args" in lib.mcgpu_last_error().decode()


def test_python_mirrors_of_the_structs_and_the_symbols():
    header = (cases.ROOT / "include" / "mcgpu_amd.h").read_text() if hasattr(cases, "ROOT") else None
    names = ["mcgpu_speedup_train_create", "mcgpu_speedup_train_step", "mcgpu_speedup_train_gradients", "mcgpu_speedup_train_predict",
             "mcgpu_speedup_train_get_state", "mcgpu_speedup_train_set_state", "mcgpu_speedup_train_destroy", "mcgpu_speedup_train_stage"]
    for name in names:
        assert name in cases.pkg.engine.ABI_SYMBOLS
        assert header is None or name + "(" in header
    if header is not None:
        for name, code in training.TRAIN_STAGES.items():
            assert f"MCGPU_SPEEDUP_TRAIN_STAGE_{name.upper()} = {code}" in header
        assert "MCGPU_SPEEDUP_PHASE_MEAN = 0, MCGPU_SPEEDUP_PHASE_VARIANCE = 1" in header
    assert "speedup_training" in cases.pkg.__all__
