// What the executors (unet.cpp, chain.cpp, ops.cpp) share at enqueue time:
// the per-call context, the layer launch helpers (exec.cpp), the U-Net's
// weight-gradient branch and its hipGraph cache.
#pragma once
#include "plan.h"

namespace hcu {

int launch_outconv_wfinalize(const float *part_oc, int R, int Co, int C, int Cs, float *dw,
                             float *db, int accumulate, hipStream_t s);
int launch_bn_count_increment(int64_t *const *ptrs, int n, hipStream_t s);

// Weight-gradient branch of the U-Net's backward: its own stream and the
// events that order it against the data-gradient chain (created on first use).
struct Branch {
  std::mutex mu;   // one user of the branch stream and its events at a time
  hipStream_t side = nullptr;
  int side_device = -1;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_slot[HCU_NBUF] = {};
  hipEvent_t ev_chain = nullptr;   // stop event of the chain's kernels (Ctx::arm_chain)
  hipEvent_t ev_prep = nullptr;    // the backward's input-gradient weight images are laid out
  hipEvent_t ev_fork_ring[HCU_FORK_RING] = {};   // marker forks (Ctx::fork)
  unsigned fork_next = 0;
  // a ring of marker events: re-recording an event whose previous record the
  // GPU has not reached yet stalls the host (config 3: ~0.9 ms per step)
  hipEvent_t next_marker() { return ev_fork_ring[fork_next++ % HCU_FORK_RING]; }
  int ensure(int dev);   // creates the stream and events on `dev` (once)
  void destroy();
  ~Branch() { destroy(); }
};

bool side_enabled();   // HCU_SIDE=0 keeps the whole backward on one stream

// Captured launch sequences (hipGraph) keyed by the buffers they bake in:
// forward and backward are fixed kernel sequences, so a replay costs one
// launch on the host instead of one per kernel.
struct GraphCache {
  struct Graph {
    std::vector<uintptr_t> key;
    hipGraphExec_t exec = nullptr;
    uint64_t used = 0;
  };
  std::mutex mu;
  std::vector<Graph> graphs;
  hipStream_t cap_stream = nullptr;
  int cap_device = -1;
  uint64_t gclock = 0;
  ~GraphCache();
  // Replays the captured launch sequence for `key`, capturing it on first use
  // (on a private stream, so nothing runs during capture) and keeping the 8
  // most recently used sequences.  A failed capture destroys `br`, whose
  // stream it may have left in an invalidated capture.
  template <class F>
  int run(std::vector<uintptr_t> key, hipStream_t s, Branch &br, F enqueue) {
    int dev = 0;
    HCU_HIP(hipGetDevice(&dev));
    key.push_back((uintptr_t)dev);
    std::lock_guard<std::mutex> lk(mu);
    for (auto &g : graphs)
      if (g.key == key) {
        g.used = ++gclock;
        HCU_HIP(hipGraphLaunch(g.exec, s));
        return HCU_OK;
      }
    if (int e = begin_capture(dev)) return e;
    const int e = enqueue(cap_stream);
    return end_capture(e, key, s, br);
  }

 private:
  int begin_capture(int dev);
  int end_capture(int enqueue_rc, const std::vector<uintptr_t> &key, hipStream_t s, Branch &br);
};

// One enqueue of a plan on the caller's stream: the workspaces, the parameter
// and gradient buffers, the gradient slots and the weight-gradient arena.
struct Ctx {
  const PlanCore &p;
  const hcu_unet_tensors &t;
  hipStream_t s;
  char *sv, *sc;
  const float *P;
  float *G;
  // Backward only: the weight-gradient branch runs on `ws` (== s when not
  // split).  It reads gradient slots the main chain has finished and writes
  // only its own partials (wpart) and the parameter gradients, so the one
  // hazard is the main chain reusing a slot the branch has not read yet.
  Branch *br;
  hipStream_t ws = nullptr;
  bool split = false;
  int next_slot = 0;
  unsigned slot_read = 0;   // slots whose last reader event was recorded in this enqueue
  float *fptr(char *base, size_t off) const { return reinterpret_cast<float *>(base + off); }
  // Base of the packed weight images (offsets wf_off / wd_off / wph_off): the
  // saved workspace, or a layer chain's caller-owned image buffer
  // (hcu_chain_forward_images), which then starts at plan offset img_lo.
  char *wi = nullptr;
  // branch: the U-Net's, when the enqueue is split over its side stream (a
  // chain has none); images: a layer chain's caller-owned weight-image buffer
  // (null: the images are in `saved`)
  Ctx(const PlanCore &plan, const hcu_unet_tensors &tensors, hipStream_t stream, Branch *branch = nullptr,
      void *images = nullptr)
      : p(plan), t(tensors), s(stream), sv((char *)tensors.saved), sc((char *)tensors.scratch),
        P(tensors.params), G(tensors.grads), br(branch), ws(branch ? branch->side : stream),
        split(branch != nullptr), wi(images ? (char *)images - plan.img_lo : nullptr) {}
  char *wimg() const { return wi ? wi : sv; }
  float *image(size_t off) const { return fptr(wimg(), off); }
  // Lays out the weight images of `n` of the plan's jobs on `stream`.
  int prep(const PrepJob *jobs, size_t n, hipStream_t stream) const {
    return launch_prep_all(P, reinterpret_cast<float *>(wimg()), jobs, (int)n, stream);
  }
  int prep(const std::vector<PrepJob> &jobs, hipStream_t stream) const {
    return prep(jobs.data(), jobs.size(), stream);
  }
  // A parameter / its gradient at a plan offset; null for an absent one
  // (offset < 0: a chain layer without bias)
  const float *param(int64_t off) const { return off >= 0 ? P + off : nullptr; }
  float *grad(int64_t off) const { return off >= 0 ? G + off : nullptr; }
  int bf() const { return p.es == 2; }   // bf16 activation storage
  float *part() const { return fptr(sc, p.part_off); }
  // Weight-gradient slab arena: each layer's partial slabs stay until its
  // finalize runs; finalizes are deferred and launched together (one batched
  // kernel on the branch stream) when the next slab would not fit, and at the
  // end of the backward.  Nothing else reads or writes the arena.
  size_t wp_off = 0;
  std::vector<WGradFinalize> pend;
  int pend_wgf(const WGradFinalize &f);
  int flush_wgf();
  // Arena space for `floats` (flushing the deferred finalizes first if needed).
  int slab(size_t floats, float *&ptr);
  float *wprep() const { return fptr(sc, p.wprep_off); }
  float *buf(int i) const { return fptr(sc, p.buf_off[i]); }
  float *kpart() const { return fptr(sc, p.kpart_off); }
  hipStream_t wstream() const { return split ? ws : s; }
  // Fresh slot for the main chain to write; waits for the branch's last read of it.
  int alloc(int &slot);
  // Branch work issued from here on sees everything the main chain has issued.
  int fork();
  // Arms the chain record (backward): kernels launched on s from here on
  // carry ev_chain, so forks need no marker; disarmed by the destructor.
  unsigned long chain_n0 = 0;
  bool armed = false;
  void arm_chain();
  ~Ctx() {
    if (armed) chain_rec().ev = nullptr;
  }
  // The branch work issued so far is the last reader of `slot`.
  int read_done(int slot);
  int join();
};

// Brackets one hcu_unet_forward / hcu_unet_backward call for the host-side
// cost accounting (HCU_HOST_PROF): slot 2 / 3 of host_prof_add, call 0 / 1.
struct HostProfScope {
  const int call;
  const bool on = host_prof_on();
  const double t0 = on ? host_now_us() : 0.0;
  double su[2];
  long sn[2];
  explicit HostProfScope(int call_) : call(call_) {
    if (on) host_prof_snap(su, sn);
  }
  ~HostProfScope() {
    if (!on) return;
    const double dt = host_now_us() - t0;
    host_prof_add(2 + call, dt);
    host_prof_call(call, su, sn, dt);
  }
};

inline void tag(const std::string &layer, const char *phase) {
  if (timing_on()) timing_set_tag((layer + "." + phase).c_str());
}

// The tensors every forward needs, and an input dtype the plan reads.
int check_forward_tensors(const PlanCore &p, const hcu_unet_tensors *t);

GConvArgs bind_conv(const GConvArgs &plan, const float *in, const float *in_scale, const float *in_shift,
                    const float *w, const float *bias, float *out, float *stats, float *partial);
int run_conv(const GConvArgs &plan, const float *in, const float *in_scale, const float *in_shift,
             const float *w, const float *bias, float *out, float *stats, float *partial, hipStream_t s);
int convt_forward(const Ctx &c, const ConvTLayer &u, const float *in, const float *in_scale,
                  const float *in_shift, float *U);
PwArgs pw_args(const ConvLayer &L, bool dgrad, const float *in, const float *w, const float *bias, float *out);
int conv_forward(const Ctx &c, const ConvLayer &L, const float *in, const float *isc,
                 const float *ish, int training, int in_fmt = 0, float *xcl_out = nullptr);
bool fuse_bnbwd(Ctx &c, GConvArgs &a, const ConvLayer *bnl);
int finish_bn(const Ctx &c, const ConvLayer &bnl, int R, int W, float *dz, int training, int accumulate);
int convt_dgrad(Ctx &c, const ConvTLayer &u, const float *dU, float *dP, const ConvLayer *bnl, int training,
                int accumulate, bool &fused);
int run_wgrad(Ctx &c, const WGradJob &j, const float *A, const float *a_scale, const float *a_shift,
              const float *G, float *dw, float *db, int accumulate);
WGradFinalize wgf_colsum(int mode, const float *rows, int R, int W, int Cout, float *db, int accumulate);
int conv_wgrad(Ctx &c, const ConvLayer &L, const float *A, const float *asc, const float *ash,
               const float *dy, int dy_slot, int accumulate);
int conv_backward(Ctx &c, const ConvLayer &L, const float *A, const float *asc,
                  const float *ash, const float *dy, int dy_slot, float *dA, int accumulate,
                  const ConvLayer *bnl = nullptr, int training = 1, bool *bn_done = nullptr,
                  float *colsum = nullptr, bool wg_late = false);
int bn_backward(const Ctx &c, const ConvLayer &L, float *dbuf, const float *pool_dP,
                const int *pool_k, int training, int accumulate);

}  // namespace hcu
