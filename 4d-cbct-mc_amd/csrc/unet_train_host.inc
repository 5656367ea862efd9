// unet_train_host.inc -- the host half that speedup_train.hip (2-D) and segment_train.hip (3-D) share of a trainer: the runner of a
// training pass, one FlexUNet with both packings and its buffers, the reverse walk of NetPass::forward, the device state of a handle
// (weights, moments, gradient, scratch) with Adam and the host <-> device copies, the tail of a report and the two stages that are the
// same operator in both.  Included inside each file's unnamed namespace, after unet_common.inc, unet_train_common.inc and the file's
// own kernels and launches (launch_wgrad needs unet_train_common.inc's launch_wgrad_fold, this file needs launch_wgrad: two include
// points).  Before the include each file gives:
//   Dims, kTaps, Report (its mcgpu_*_train_report);
//   launch_conv, launch_maxpool (its *_conv.inc);
//   launch_wgrad(RunnerBase<Report>&, c_out, src1, c1, src2, c2, ups, D, dy, part, grad_w, grad_b, scale), wgrad_plan and
//     wgrad_part_floats(c_in, c_out, D), launch_maxpool_backward(x, dy, dx, C, D);
//   Dgrad: the input-gradient GEMM or GEMMs of one layer.  Dgrad() is none; Dgrad(const ConvLayer&, int c1) those of a layer whose
//     first source has c1 channels; each(f) visits its GEMMs as ConvLayers (the owner gives each its wpack and a bias of zeros);
//     pack(const ConvLayer&, const float* d_w) packs them from the layer's weights; with it
//     launch_dgrad(const Dgrad&, dy, D, ext, ups, out1, out2) and dgrad_ext_floats(const ConvLayer&, int c1, const Dims&), the floats of
//     `ext` that launch_dgrad needs for the layer.

// Launches of a trainer.  The forward pass is NetPass::forward with this runner: norm_lrelu gives every normed layer of the pass
// its own sums, in the order of the pass, for the backward to find.  Whole passes are timed, not single launches.
struct TrainRunner : RunnerBase<Report> {
  std::vector<double2*>* norm_parts = nullptr;  // of the net whose forward runs
  size_t norm_i = 0;

  void conv(const ConvLayer& l, const float* src1, int c1, const float* src2, int ups, const Dims& D, float* out) { launch_conv(l, src1, c1, src2, ups, D, out); }
  void maxpool(const float* x, float* y, int C, const Dims& D) { launch_maxpool(x, y, C, D); }
  void norm_lrelu(const float* x, float* y, int C, size_t n) {
    double2* part = norm_parts ? (*norm_parts)[norm_i++] : d_part;
    stats(x, C, n, part);
    hipLaunchKernelGGL(norm_lrelu_kernel, dim3(blocks_of(n), (unsigned)C), dim3(256), 0, nullptr, x, y, n, segments_of(n), part);
  }
};

void launch_pack_forward(const ConvLayer& l, const float* d_w) {
  const size_t total = l.pack_floats();
  hipLaunchKernelGGL(pack_weights_kernel<kTaps>, dim3(blocks_of(total)), dim3(256), 0, nullptr, d_w, l.wpack, l.c_in, l.c_out, l.n_chunks, 32 * l.nb, total);
}

// One FlexUNet of a trainer: its layers with both packings, the buffers of a forward pass and, mirrored, of the gradients
struct TrainNet {
  NetLayers layers;
  size_t w_begin, w_end;        // its range of the flat weights
  std::vector<Dgrad> dgrad;     // in the order of NetLayers::each; init_conv has none
  std::vector<double2*> parts;  // the sums of each normed layer, in the order of the forward pass
  std::unique_ptr<NetPass<TrainRunner, Dims>> act, grad;
  size_t part_floats = 0, ext_floats = 0;

  TrainNet(NetLayers made, TrainRunner& R, const Dims& P, float* d_w, const float* d_zero) : layers(std::move(made)), dgrad(2 + 4 * layers.L) {
    const int L = layers.L;
    w_begin = w_end = layers.init.w_off;
    size_t k = 0;
    auto place = [&](ConvLayer& l, int c1, const Dims& D) {  // c1: channels of the first source; 0: no input gradient is needed
      w_end = std::max(w_end, l.b_off + (size_t)l.c_out);
      l.wpack = (float*)R.alloc_bytes(l.pack_floats() * sizeof(float), false);
      l.bias = d_w + l.b_off;
      part_floats = std::max(part_floats, wgrad_part_floats(l.c_in, l.c_out, D));
      Dgrad& g = dgrad[k++];
      if (!c1) return;
      g = Dgrad(l, c1);
      g.each([&](ConvLayer& m) {
        m.wpack = (float*)R.alloc_bytes(m.pack_floats() * sizeof(float), false);
        m.bias = d_zero;
      });
      ext_floats = std::max(ext_floats, dgrad_ext_floats(l, c1, D));
    };
    place(layers.init, 0, P);
    place(layers.final, layers.final.c_in, P);
    for (int i = 0; i < 2 * L; ++i) place(layers.enc[i], layers.enc[i].c_in, P.shifted(i / 2 + 1));
    for (int i = 0; i < 2 * L; ++i) place(layers.dec[i], i % 2 ? layers.dec[i].c_in : layers.skip_c[i / 2], P.shifted(i / 2));
    act.reset(new NetPass<TrainRunner, Dims>(layers, R, P));
    grad.reset(new NetPass<TrainRunner, Dims>(layers, R, P));
    auto sums = [&](int c) { parts.push_back((double2*)R.alloc_bytes((size_t)c * kMaxSegments * sizeof(double2), true)); };
    for (int i = 0; i < L; ++i) { sums(layers.skip_c[i + 1]); sums(layers.skip_c[i + 1]); }
    for (int i = L - 1; i >= 0; --i) { sums(layers.dec_c[i]); sums(layers.dec_c[i]); }
  }
  void pack(const float* d_w) {
    size_t k = 0;
    layers.each([&](ConvLayer& l) {
      launch_pack_forward(l, d_w + l.w_off);
      dgrad[k++].pack(l, d_w + l.w_off);
    });
  }
  const Dgrad& dgrad_final() const { return dgrad[1]; }
  const Dgrad& dgrad_enc(int k) const { return dgrad[2 + k]; }  // of layers.enc[k]
  const Dgrad& dgrad_dec(int k) const { return dgrad[2 + 2 * layers.L + k]; }
  // the sums of the k-th normed layer of the forward pass: enc_i first, second = 2 i, 2 i + 1; dec_i = 2 L + 2 (L - 1 - i) (+ 1)
  double2* enc_part(int i, int second) { return parts[2 * i + second]; }
  double2* dec_part(int i, int second) { return parts[2 * layers.L + 2 * (layers.L - 1 - i) + second]; }
};

// What a handle keeps on the device beside its nets: the flat weights, both moments, the batch gradient, the zeros that are the bias
// of every input-gradient GEMM, and the scratch of a backward pass
struct TrainCore {
  TrainRunner* R = nullptr;
  int device = 0;
  size_t n_w = 0;
  float *d_w = nullptr, *d_m1 = nullptr, *d_m2 = nullptr, *d_grad = nullptr, *d_zero = nullptr, *d_part = nullptr, *d_ext = nullptr;
  double2* d_bpart = nullptr;

  // widest: the most channels of a layer
  void alloc(TrainRunner& runner, int dev, const float* weights, size_t n_weights, int widest) {
    R = &runner;
    device = dev;
    n_w = n_weights;
    d_w = R->upload(weights, n_w);
    d_m1 = R->alloc(n_w);
    d_m2 = R->alloc(n_w);
    d_grad = R->alloc(n_w);
    d_zero = R->alloc((size_t)2 * widest + 2);  // as many as the widest concatenated input has channels
    d_bpart = (double2*)R->alloc_bytes((size_t)widest * kMaxSegments * sizeof(double2), true);
  }
  void alloc_scratch(size_t part_floats, size_t ext_floats) {
    d_part = R->alloc(part_floats);
    d_ext = R->alloc(ext_floats);
  }
  size_t planned_bytes() const { return R->dry ? R->planned : R->dev.held; }

  void check_live(const char* fn) const {
    if (R->dry) refuse(fn, "the handle is a dry plan: nothing runs on it");
    HIP_TRY(hipSetDevice(device));
  }
  template <class State>
  void check_state(const char* fn, const State& s) const {
    if ((s.weights || s.moment1 || s.moment2) && s.n_weights != n_w)
      refuse(fn, "n_weights is " + std::to_string(s.n_weights) + " but the trainer has " + std::to_string(n_w) + " values");
  }

  // both packings of `nets` from the weights as they are now; waits for the device
  void repack(std::initializer_list<TrainNet*> nets) const {
    for (TrainNet* N : nets) N->pack(d_w);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
  }
  // one Adam update of the net's range of the weights, then both of its packings again
  void update(TrainNet& N, double lr, double beta1, double beta2, unsigned long long t) const {
    launch_adam(d_w + N.w_begin, d_grad + N.w_begin, d_m1 + N.w_begin, d_m2 + N.w_begin, N.w_end - N.w_begin, lr, beta1, beta2, t);
    N.pack(d_w);
  }
  // the arrays that the state names, to the host
  template <class State>
  void get_arrays(const char* fn, const State& s) const {
    if (!(s.weights || s.moment1 || s.moment2)) return;
    check_live(fn);
    if (s.weights) HIP_TRY(hipMemcpy(s.weights, d_w, n_w * 4, hipMemcpyDeviceToHost));
    if (s.moment1) HIP_TRY(hipMemcpy(s.moment1, d_m1, n_w * 4, hipMemcpyDeviceToHost));
    if (s.moment2) HIP_TRY(hipMemcpy(s.moment2, d_m2, n_w * 4, hipMemcpyDeviceToHost));
  }
  // and from the host; weights that came in are packed again
  template <class State>
  void set_arrays(const char* fn, const State& s, std::initializer_list<TrainNet*> nets) const {
    if (!(s.weights || s.moment1 || s.moment2)) return;
    check_live(fn);
    if (s.weights) HIP_TRY(hipMemcpy(d_w, s.weights, n_w * 4, hipMemcpyHostToDevice));
    if (s.moment1) HIP_TRY(hipMemcpy(d_m1, s.moment1, n_w * 4, hipMemcpyHostToDevice));
    if (s.moment2) HIP_TRY(hipMemcpy(d_m2, s.moment2, n_w * 4, hipMemcpyHostToDevice));
    if (s.weights) repack(nets);
  }
};

// The gradient of one sample added to C.d_grad: NetPass::forward walked in reverse.  x: the net's input; grad->out holds dL/d(output).
void backward_sample(TrainRunner& R, TrainNet& N, const float* x, const TrainCore& C, double scale) {
  NetLayers& net = N.layers;
  auto& A = *N.act;
  auto& G = *N.grad;
  const int L = net.L;
  const Dims P = A.P;
  auto wgrad = [&](const ConvLayer& l, const float* s1, int c1, const float* s2, int ups, const Dims& D, const float* dy, bool bias) {
    Stage st(R.dev, R.rep.ms_wgrad);
    launch_wgrad(R, l.c_out, s1, c1, s2, l.c_in - c1, ups, D, dy, C.d_part, C.d_grad + l.w_off, bias ? C.d_grad + l.b_off : nullptr, scale);
    st.done();
  };
  auto dgrad = [&](const Dgrad& d, const float* dy, const Dims& D, int ups, float* o1, float* o2) {
    Stage st(R.dev, R.rep.ms_dgrad);
    launch_dgrad(d, dy, D, C.d_ext, ups, o1, o2);
    st.done();
  };
  auto norm = [&](const float* y, float* dy, int c, const Dims& D, const double2* fpart) {
    Stage st(R.dev, R.rep.ms_norm);
    launch_norm_backward(y, dy, c, D.voxels(), fpart, C.d_bpart);
    st.done();
  };
  wgrad(net.final, A.dec_b[0], net.final.c_in, nullptr, 0, P, G.out, true);
  dgrad(N.dgrad_final(), G.out, P, 0, G.dec_b[0], nullptr);
  for (int i = 0; i < L; ++i) {
    const Dims D = P.shifted(i);
    const int c = net.dec_c[i];
    const float* cur = i == L - 1 ? A.skip[L] : A.dec_b[i + 1];
    float* g_cur = i == L - 1 ? G.skip[L] : G.dec_b[i + 1];
    norm(A.dec_b[i], G.dec_b[i], c, D, N.dec_part(i, 1));
    wgrad(net.dec[2 * i + 1], A.dec_a[i], c, nullptr, 0, D, G.dec_b[i], false);
    dgrad(N.dgrad_dec(2 * i + 1), G.dec_b[i], D, 0, G.dec_a[i], nullptr);
    norm(A.dec_a[i], G.dec_a[i], c, D, N.dec_part(i, 0));
    wgrad(net.dec[2 * i], A.skip[i], net.skip_c[i], cur, 1, D, G.dec_a[i], false);
    dgrad(N.dgrad_dec(2 * i), G.dec_a[i], D, 1, G.skip[i], g_cur);
  }
  for (int i = L - 1; i >= 0; --i) {
    const Dims D = P.shifted(i + 1);
    const int c = net.skip_c[i + 1];
    norm(A.skip[i + 1], G.skip[i + 1], c, D, N.enc_part(i, 1));
    wgrad(net.enc[2 * i + 1], A.enc_a[i], c, nullptr, 0, D, G.skip[i + 1], false);
    dgrad(N.dgrad_enc(2 * i + 1), G.skip[i + 1], D, 0, G.enc_a[i], nullptr);
    norm(A.enc_a[i], G.enc_a[i], c, D, N.enc_part(i, 0));
    wgrad(net.enc[2 * i], A.pooled[i], net.skip_c[i], nullptr, 0, D, G.enc_a[i], false);
    dgrad(N.dgrad_enc(2 * i), G.enc_a[i], D, 0, G.pooled[i], nullptr);
    {
      Stage st(R.dev, R.rep.ms_dgrad);
      launch_maxpool_backward(A.skip[i], G.pooled[i], G.skip[i], net.skip_c[i], P.shifted(i));
      st.done();
    }
  }
  wgrad(net.init, x, net.in_channels, nullptr, 0, P, G.skip[0], true);
}

// --------------------------------------------------------------------------------------------------------------- the report
void clear_times(Report& r) { r.ms_forward = r.ms_wgrad = r.ms_dgrad = r.ms_norm = r.ms_optimizer = r.ms_total = 0.0; }

// the peak, the time since t0 and the report to the caller
void finish_report(RunnerBase<Report>& R, const std::chrono::steady_clock::time_point& t0, Report* report) {
  R.rep.peak_device_bytes = R.dev.peak;
  R.rep.ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  mcgpu::write_report(report, R.rep);
}

// ---------------------------------------------------------------------------------------------------------------- the stages
// The two backward operators that are the same call in both nets, each alone for mcgpu_*_train_stage, beside unet_common.inc's
// stage_conv and stage_maxpool: `a` is the stage's arguments, D the extent of a.in
template <class Args>
void stage_wgrad(TrainRunner& R, const Args& a, const Dims& D) {
  const Dims E = a.upsample ? D.halved_up() : D;
  const size_t n = D.voxels();
  const int c_in = a.c1 + a.c2;
  const float* d_in = R.upload(a.in, (size_t)a.c1 * n);
  const float* d_in2 = a.c2 ? R.upload(a.in2, (size_t)a.c2 * E.voxels()) : nullptr;
  const float* d_dy = R.upload(a.in3, (size_t)a.c_out * n);
  float* d_part = R.alloc(wgrad_part_floats(c_in, a.c_out, D));
  const size_t n_w = (size_t)a.c_out * c_in * kTaps;
  float* d_grad = R.alloc(n_w + a.c_out);
  Stage st(R.dev, R.rep.ms_wgrad);
  launch_wgrad(R, a.c_out, d_in, a.c1, d_in2, a.c2, a.upsample, D, d_dy, d_part, d_grad, d_grad + n_w, 1.0);
  st.done();
  HIP_TRY(hipMemcpy(a.out, d_grad, n_w * 4, hipMemcpyDeviceToHost));
  if (a.out2) HIP_TRY(hipMemcpy(a.out2, d_grad + n_w, (size_t)a.c_out * 4, hipMemcpyDeviceToHost));
  if (a.values) a.values[0] = (double)wgrad_plan(c_in, a.c_out, D).partials();
}

// dx0: what the skip's gradient holds before the pool's is added (host, [c1][D]), or nullptr for zeros
template <class Args>
void stage_maxpool_backward(TrainRunner& R, const Args& a, const Dims& D, const float* dx0) {
  const size_t n = D.voxels();
  const float* d_x = R.upload(a.in, (size_t)a.c1 * n);
  const size_t n_dy = (size_t)a.c1 * D.shifted(1).voxels();
  const float* d_dy = R.upload(a.in2, std::max<size_t>(n_dy, 1));
  float* d_dx = dx0 ? R.upload(dx0, (size_t)a.c1 * n) : R.alloc((size_t)a.c1 * n);
  Stage st(R.dev, R.rep.ms_dgrad);
  launch_maxpool_backward(d_x, d_dy, d_dx, a.c1, D);
  st.done();
  HIP_TRY(hipMemcpy(a.out, d_dx, (size_t)a.c1 * n * 4, hipMemcpyDeviceToHost));
}
