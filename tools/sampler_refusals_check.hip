// Host-only check of the sampler's refusals (sample_refusals in kandinsky-5_amd/csrc/engine.hip) under AddressSanitizer and UBSan: the function
// makes no HIP call and touches no handle state, so it runs on a machine without a GPU, on a default-constructed handle, with fake non-null
// pointers that are never dereferenced and real host arrays for the window starts.  The engine source is included whole (the handle's
// struct lives there); the other objects of the library are linked as built:
//
//   python kandinsky-5_amd/build.py
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -w -I include -I kandinsky-5_amd/csrc -Xarch_host -fsanitize=address,undefined \
//       -c tools/sampler_refusals_check.hip -o /tmp/sampler_refusals_check.o
//   hipcc --offload-arch=gfx950 -fsanitize=address,undefined /tmp/sampler_refusals_check.o \
//       $(ls kandinsky-5_amd/build/*.o | grep -v /engine.o) -ldl -o /tmp/sampler_refusals_check
//   /tmp/sampler_refusals_check          (prints one line per case; exit status 0 = every status and message as expected)
#include "engine.hip"

#include <cstdio>

static int failures = 0;

static void expect(const char* what, int got, int want, const char* message) {
  const bool ok = got == want && (!message || strstr(k5_last_error(), message));
  printf("%-46s status %d %s%s\n", what, got, ok ? "ok" : "UNEXPECTED: ", ok ? "" : k5_last_error());
  failures += !ok;
}

int main() {
  k5_dit* d = new k5_dit();
  d->cfg.in_visual_dim = d->cfg.out_visual_dim = 16;
  d->cfg.visual_cond = 1;
  const int T = 3, H = 8, W = 12;
  const uintptr_t bytes = (uintptr_t)T * H * W * 16 * 4;
  const uintptr_t base = 0x10000000;                       // fake device addresses, never dereferenced
  float sigmas[5] = {1.0f, 0.75f, 0.5f, 0.25f, 0.0f};
  k5_sample_args a{};
  a.fwd.T = T; a.fwd.H = H; a.fwd.W = W;
  a.latent = reinterpret_cast<float*>(base); a.sigmas = sigmas; a.num_steps = 4; a.guidance_weight = 5.0f;
  auto at = [](uintptr_t p) { return reinterpret_cast<float*>(p); };
  auto run = [&](const k5_edit_args* e, const k5_sample_windows_args* w) { g_err[0] = 0; return sample_refusals(d, &a, nullptr, e, w, "check"); };

  expect("plain, aligned latent", run(nullptr, nullptr), K5_OK, nullptr);
  expect("null arguments", sample_refusals(d, nullptr, nullptr, nullptr, nullptr, "check"), K5_ERR_ARG, nullptr);
  g_err[0] = 0;
  expect("visual_cond misaligned", sample_refusals(d, &a, at(base + 2 * bytes + 2), nullptr, nullptr, "check"), K5_ERR_ARG, "visual_cond is not 4-byte aligned");

  k5_edit_args e{};
  e.source = at(base + 2 * bytes); e.noise = at(base + 4 * bytes); e.keep_mask = at(base + 6 * bytes);
  expect("edit, aligned and apart", run(&e, nullptr), K5_OK, nullptr);
  a.latent = at(base + 2);
  expect("edit, misaligned latent", run(&e, nullptr), K5_ERR_ARG, "latent is not 4-byte aligned");
  a.latent = at(base);
  e.source = at(base + bytes - 4);
  expect("edit, source overlaps the latent's last cell", run(&e, nullptr), K5_ERR_ARG, "edit source overlaps latent");
  e.source = at(base + 2 * bytes); e.noise = at(base - bytes + 4);
  expect("edit, noise overlaps the latent's first cell", run(&e, nullptr), K5_ERR_ARG, "edit noise overlaps latent");
  e.noise = at(base + 4 * bytes); e.keep_mask = at(base + 64);
  expect("edit, keep_mask inside the latent", run(&e, nullptr), K5_ERR_ARG, "edit keep_mask overlaps latent");
  e.keep_mask = at(base + bytes);
  expect("edit, keep_mask right after the latent", run(&e, nullptr), K5_OK, nullptr);
  e.keep_mask = at(base + 6 * bytes + 1);
  expect("edit, keep_mask misaligned", run(&e, nullptr), K5_ERR_ARG, "edit keep_mask is not 4-byte aligned");

  float weights[65 * 3];
  for (float& v : weights) v = 1.0f;
  int starts[65];
  k5_sample_windows_args w{};
  w.sample = a; w.weights = weights; w.starts = starts;
  auto windows = [&](int nwin, int F, int total_T) {
    w.nwin = nwin; w.total_T = total_T; w.sample.fwd.T = F;
    g_err[0] = 0;
    return sample_refusals(d, &w.sample, nullptr, nullptr, &w, "check");
  };
  for (int i = 0; i < 65; ++i) starts[i] = i;
  expect("windows, nwin 0", windows(0, 2, 65), K5_ERR_ARG, "nwin must be 1..64 (got 0)");
  expect("windows, nwin 1", windows(1, 3, 3), K5_OK, nullptr);
  expect("windows, nwin 64", windows(64, 2, 65), K5_OK, nullptr);
  expect("windows, nwin 65", windows(65, 2, 66), K5_ERR_ARG, "nwin must be 1..64 (got 65)");
  starts[0] = 0; starts[1] = 3; starts[2] = 1;
  expect("windows, descending starts", windows(3, 3, 6), K5_ERR_ARG, "starts must ascend");
  starts[1] = 1; starts[2] = 5;
  expect("windows, a gap in coverage", windows(3, 3, 8), K5_ERR_ARG, "no window covers frame 4");
  starts[2] = 3;
  expect("windows, the end uncovered", windows(3, 3, 7), K5_ERR_ARG, "no window covers frame 6");
  expect("windows, a window past total_T", windows(3, 3, 5), K5_ERR_ARG, "reaches outside the 5 frames");
  expect("windows, the plan of (6, 3, 1)", windows(3, 3, 6), K5_OK, nullptr);
  expect("windows with an edit", (g_err[0] = 0, sample_refusals(d, &w.sample, nullptr, &e, &w, "check")), K5_ERR_ARG, "keep_mask is not 4-byte aligned");
  e.keep_mask = nullptr;
  expect("windows with an edit, aligned", (g_err[0] = 0, sample_refusals(d, &w.sample, nullptr, &e, &w, "check")), K5_ERR_UNSUPPORTED, "editing with context windows");
  d->watch.on = true; d->watch.every = 2;
  expect("windows under a watch with previews", windows(3, 3, 6), K5_ERR_STATE, "the watch has previews (preview_every = 2)");
  delete d;
  printf("%d unexpected\n", failures);
  return failures ? 1 : 0;
}
