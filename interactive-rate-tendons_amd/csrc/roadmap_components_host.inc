// roadmap_components_host.inc -- part of roadmap.hip: component labels of the roadmap minus the items known invalid (kernels: roadmap_kernel.hpp).
namespace {

void free_comp(tr_roadmap *r) {
  if (r->dc.arena) dev_cache().release(r->dc.arena);
  r->dc = tr_roadmap::DevComp{};
}

// The same labels on one host thread: for the searches the kernel hands back WHILE it runs, when the device cannot be asked (its stream
// is busy with the searches).  Only equality of two labels is ever used.
void host_component_labels(tr_roadmap *r) { host_components(r, true, r->dc.label); }

// r->dc.label[v] = the smallest vertex of v's component in the graph minus the items known invalid.  false: not available (no
// edges, out of memory): the caller searches as before.
bool component_labels(tr_roadmap *r, const RoadmapSwitches &sw) {
  auto &c = r->dc;
  c.status_current = false;
  if (c.state < 0 || r->E == 0 || r->V < 2) return false;
  const int dev = tr_device(r->ctx);
  const int64_t V = r->V, E = r->E;
  if (hipSetDevice(dev) != hipSuccess) return false;
  if (c.state == 0) {
    c.state = -1;
    const size_t b_e = up((size_t)E * 4), b_v = up((size_t)V * 4), b_vs = up((size_t)V), b_es = up((size_t)E);
    if (dev_cache().alloc(dev, (void **)&c.arena, 2 * b_e + 2 * b_v + b_vs + b_es) != hipSuccess) return false;
    char *p = c.arena;
    c.d_eu = (int32_t *)p; p += b_e;
    c.d_ev = (int32_t *)p; p += b_e;
    c.d_parent = (int32_t *)p; p += b_v;
    c.d_label = (int32_t *)p; p += b_v;
    c.d_vstat = (uint8_t *)p; p += b_vs;
    c.d_estat = (uint8_t *)p;
    if (hipMemcpyAsync(c.d_eu, r->eu.data(), (size_t)E * 4, hipMemcpyHostToDevice, nullptr) != hipSuccess ||
        hipMemcpyAsync(c.d_ev, r->ev.data(), (size_t)E * 4, hipMemcpyHostToDevice, nullptr) != hipSuccess) { free_comp(r); r->dc.state = -1; return false; }
    c.label.resize((size_t)V);
    c.state = 1;
  }
  bool ok = hipMemcpyAsync(c.d_vstat, r->vstat.data(), (size_t)V, hipMemcpyHostToDevice, nullptr) == hipSuccess &&
            hipMemcpyAsync(c.d_estat, r->estat.data(), (size_t)E, hipMemcpyHostToDevice, nullptr) == hipSuccess;
  if (!ok) return false;
  const bool timing = sw.stats;
  const auto t0 = Clock::now();
  if (timing) (void)hipStreamSynchronize(nullptr);
  const auto t1 = Clock::now();
  hipLaunchKernelGGL(cc_init, dim3((unsigned)((V + 255) / 256)), dim3(256), 0, nullptr, c.d_parent, V);
  hipLaunchKernelGGL(cc_seed, dim3((unsigned)((E + 255) / 256)), dim3(256), 0, nullptr, c.d_eu, c.d_ev, c.d_estat, c.d_vstat, E, c.d_parent);
  hipLaunchKernelGGL(cc_hook, dim3((unsigned)((E + 255) / 256)), dim3(256), 0, nullptr, c.d_eu, c.d_ev, c.d_estat, c.d_vstat, E, c.d_parent);
  hipLaunchKernelGGL(cc_flatten, dim3((unsigned)((V + 255) / 256)), dim3(256), 0, nullptr, c.d_parent, c.d_label, V);
  if (hipGetLastError() != hipSuccess) return false;
  if (timing) (void)hipStreamSynchronize(nullptr);
  const auto t2 = Clock::now();
  if (hipMemcpy(c.label.data(), c.d_label, (size_t)V * 4, hipMemcpyDeviceToHost) != hipSuccess) return false;
  if (timing)
    std::fprintf(stderr, "[tendon_hip] component labels: validity bytes up %.3f ms, kernels %.3f ms, labels down %.3f ms\n", ms_between(t0, t1), ms_between(t1, t2),
                 ms_between(t2, Clock::now()));
  c.status_current = true;
  return true;
}

}  // namespace
