// netvlad_host.hip -- host side of NetVLAD (include/d2fe.h: d2fe_load_netvlad .. d2fe_netvlad): the layer descriptors, the execution plan, the
// weight packing of every plan step and the launch sequence run_netvlad.  The kernels live in netvlad.hip, netvlad_fused.hip and netvlad_pair.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "context.h"
#ifdef D2FE_DEVTOOLS
#include "../../include/d2fe_debug.h"
#endif

using namespace d2fe;

namespace d2fe {
NvNet::~NvNet() {
  for (auto& l : layers) for (float* p : {l.w, l.b}) if (p) hipFree(p);
  for (auto& st : plan) for (float* p : {st.w0, st.we, st.wp, st.bp, st.wp2, st.bp2}) if (p) hipFree(p);
  for (float* p : {pre_w, pre_b, aw, aw_pack, ab, cen, pca_comp, pca_mean}) if (p) hipFree(p);
}

int NvRun::alloc(const NvNet& net, int B) {
  release();
  out.assign(net.layers.size(), nullptr);
  last = {std::vector<NvSlabs>(net.layers.size()), NvSlabs(), 0};
  for (size_t li = 0; li < net.layers.size(); ++li)
    if (net.layers[li].materialised) HIP_TRY(hipMalloc(&out[li], sizeof(float) * (size_t)net.layers[li].gmax * B * net.layers[li].oh * net.layers[li].ow * net.layers[li].cout));
  const int ch = net.layers.back().oh, cw = net.layers.back().ow;
  HIP_TRY(hipMalloc(&feat_buf, sizeof(float) * (size_t)net.feat_gmax * B * ch * cw * net.proj));
  HIP_TRY(hipMalloc(&raw, sizeof(float) * (size_t)B * net.k * net.proj));
  HIP_TRY(hipMalloc(&part, sizeof(float) * (size_t)B * nv_vlad_part_floats(ch * cw, net.proj, net.k)));
  return D2FE_OK;
}

void NvRun::release() {
  for (float* p : out) if (p) hipFree(p);
  out.clear();
  for (float** p : {&feat_buf, &raw, &part}) if (*p) { hipFree(*p); *p = nullptr; }
  if (stamps) { hipFree(stamps); stamps = nullptr; }
}
}  // namespace d2fe

namespace {

inline int same_out(int in, int stride) { return (in + stride - 1) / stride; }
inline int same_pad_begin(int in, int stride, int out) { const int t = (out - 1) * stride + 3 - in; return t > 0 ? t / 2 : 0; }   // TF "SAME", 3x3

// hidden-channel groups for a fused step: enough workgroups to fill the chip (2 per CU), at least 3 chunks of 16 per group (every
// group stages the whole input patch again, and its consumer reads one more partial slab).  Three or more groups (two, when the consumer reads a
// single slab: `sum_at_2`) cost a slab-sum launch of ~6 us behind the block; a chunk costs ~2.3 us of a workgroup's latency (tools/nv_stamps.py):
// the split goes past two groups only when the chunks it takes off every workgroup are worth more than that launch (30 x 40 layers: 9-12 chunks,
// two groups; 15 x 20 layers: 60 chunks, seven)
inline void nv_groups(long base_blocks, int nchunk, int gmax, int* groups, int* cpg, int target, long cap = 0, bool sum_at_2 = false, bool rule = true) {
  int g = (int)((target + base_blocks - 1) / base_blocks);
  if (cap > 0 && g > 1 && g * base_blocks > cap) --g;      // a second round of workgroups costs more than one more chunk per group
  if (g > gmax) g = gmax;
  if (g > nchunk / 3) g = nchunk / 3;
  if (g < 1) g = 1;
  auto per = [&](int gg) { return (nchunk + gg - 1) / gg; };
  const double chunk_us = 2.3, launch_us = 6.0;
  if (rule && g >= 3 && (per(2) - per(g)) * chunk_us < launch_us) g = 2;
  if (rule && g == 2 && sum_at_2 && (per(1) - per(2)) * chunk_us < launch_us) g = 1;
  // round 6 (MobileNetV2-0.75: 9 chunks at 120 x 160 and 60 x 80): with 32 or more tiles per image a second group halves a workgroup's chunks (~10 us of ONE image's
  // latency) but makes every batch stage each input patch twice, write and re-read a second slab and, where the consumer wants one slab, launch the slab sum:
  // measured at 32 images 194 + 26 us with two groups against 160 us with one (profiles/r06_netvlad_timeline.txt).  The split stays per IMAGE (batch invariance)
  if (rule && g == 2 && base_blocks >= 32 && nchunk <= 12) g = 1;
  *cpg = per(g);
  *groups = (nchunk + *cpg - 1) / *cpg;
}

// layer list -> descriptors with the output size of each layer at a H x W input; checks what every launch form needs (no HIP calls).
// need_weights = false: the weight pointers may be null (the plan alone)
int nv_describe(const d2fe_nv_layer* layers, int n_layers, int H, int W, bool need_weights, std::vector<NvLayer>* out) {
  int ch = H, cw = W, cprev = 1;
  out->clear();
  for (int i = 0; i < n_layers; ++i) {
    const d2fe_nv_layer& L = layers[i];
    NvLayer l{L.kind, L.cin, L.cout, 0, L.stride, L.act, L.res};
    if ((need_weights && (!L.weight || !L.bias)) || L.stride < 1 || L.stride > 2 || L.cin != cprev || L.res >= i || L.act < 0 || L.act > 2)
      return fail(D2FE_ERR_INVALID, "netvlad layer " + std::to_string(i) + ": bad descriptor");
    if (L.kind == D2FE_NV_CONV) {
      if (i != 0 || L.cin != 1 || L.cout > 32) return fail(D2FE_ERR_INVALID, "conv layer must be first, 1 -> <=32 channels");
      l.cout_pad = 32;
    } else if (L.kind == D2FE_NV_DW) {
      if (L.cin != L.cout || (L.cin & 3)) return fail(D2FE_ERR_INVALID, "depthwise layer: channels must match and be a multiple of 4");
      l.cout_pad = L.cout;
    } else if (L.kind == D2FE_NV_PW) {
      if ((L.cin & 3) || L.stride != 1) return fail(D2FE_ERR_INVALID, "pointwise layer: cin must be a multiple of 4, stride 1");
      if (L.cin & 7) return fail(D2FE_ERR_INVALID, "pointwise layer: cin must be a multiple of 8");
      l.cout_pad = (L.cout + 31) / 32 * 32;
    } else {
      return fail(D2FE_ERR_INVALID, "unknown layer kind");
    }
    ch = same_out(ch, L.stride); cw = same_out(cw, L.stride);
    l.oh = ch; l.ow = cw;
    if (L.res >= 0) {
      // a skip connection adds two tensors of the SAME shape: channels and spatial size (a stride-2 layer in between would make
      // the 1x1 kernel read past the smaller buffer)
      const auto& r = (*out)[L.res];
      if (L.kind != D2FE_NV_PW || r.cout != L.cout || r.oh != ch || r.ow != cw)
        return fail(D2FE_ERR_INVALID, "netvlad layer " + std::to_string(i) + ": residual source has a different shape");
    }
    out->push_back(l);
    cprev = L.cout;
  }
  return D2FE_OK;
}

// The execution plan: fuse [conv0 ->] [pw expand ->] dw -> pw project where the kernels support the shape (knobs.legacy: one launch per layer), in the
// pattern order front block -> expand block -> dw + pw -> tail.  Marks the materialised layers and the slab room (gmax) of every block output.  Pure host
// code.  Returns -1, or the index of a layer whose residual source would be internal to a fused block
int nv_plan(std::vector<NvLayer>& L, int proj_dim, const NvKnobs& kn, std::vector<NvStep>* plan) {
  const int nl = (int)L.size();
  auto K = [&](int i) { return i < nl ? L[i].kind : -1; };
  const NvKind single[3] = {NvKind::Conv0, NvKind::Pw, NvKind::Dw};      // by d2fe_nv_kind
  plan->clear();
  for (int i = 0; i < nl;) {
    NvStep st;
    st.kind = single[L[i].kind]; st.l0 = st.l1 = i;
    if (!kn.legacy) {
      if (K(i) == D2FE_NV_CONV && K(i + 1) == D2FE_NV_DW && K(i + 2) == D2FE_NV_PW && L[i + 1].res < 0 && L[i + 2].res < 0) {
        // pixel-pair form (netvlad_pair.hip): the first block with a first conv of 16 / 24 / 32 channels
        if (kn.pair && nv_fpair_supported(L[i].cout, L[i].stride, L[i + 1].stride, L[i + 2].cout)) { st.kind = NvKind::FPair; st.l1 = i + 2; }
        else if (nv_block_supported(L[i + 1].cin, L[i + 1].cin, L[i + 2].cout, L[i + 1].stride, false, 1)) { st.kind = NvKind::Front; st.l1 = i + 2; }
      } else if (i > 0 && K(i) == D2FE_NV_PW && K(i + 1) == D2FE_NV_DW && K(i + 2) == D2FE_NV_PW && L[i].res < 0) {
        const int cin = L[i].cin, chid = L[i].cout, cout = L[i + 2].cout, stride = L[i + 1].stride;
        // stride 1: the pixel-pair form (netvlad_pair.hip, the widths in NVP_SHAPES); otherwise the input-in-registers form where the shape allows it,
        // the LDS-resident form of nv_block_kernel last
        if (kn.pair && nv_pblock_supported(cin, chid, cout, stride)) st.kind = NvKind::PBlock;
        else if (nv_block_supported(cin, chid, cout, stride, true, 0))
          st.kind = kn.xblock && nv_xblock_supported(cin, chid, cout, stride) ? NvKind::XBlock : NvKind::Expand;
        if (nv_fused(st.kind)) st.l1 = i + 2;
      } else if (i > 0 && K(i) == D2FE_NV_DW && K(i + 1) == D2FE_NV_PW && nv_block_supported(L[i].cin, L[i].cin, L[i + 1].cout, L[i].stride, false, 0)) {
        st.kind = NvKind::Block; st.l1 = i + 1;
      } else if (i > 0 && i == nl - 1 && K(i) == D2FE_NV_PW && L[i].res < 0) {
        // last 1x1 of the trunk + the NetVLAD pre-projection in one launch
        if (nv_tail_supported(L[i].cin, proj_dim)) st.kind = NvKind::Tail;
        else if (nv_block_supported(L[i].cin, L[i].cout, proj_dim, 1, true, 2)) st.kind = NvKind::TailBlock;
      }
      // a residual must read a tensor that exists in HBM: the output of an earlier step
      if (nv_fused(st.kind) && !nv_is_tail(st.kind) && L[st.l1].res >= 0 && !L[L[st.l1].res].materialised) { st.kind = single[L[i].kind]; st.l1 = i; }
    }
    if (!nv_fused(st.kind) && L[i].res >= 0 && !L[L[i].res].materialised) return i;
    if (st.kind == NvKind::PBlock) st.halves = nv_pblock_halves(L[st.l1].cout);
    if (nv_fused(st.kind) && !nv_is_tail(st.kind) && L[st.l1].act == 0)
      L[st.l1].gmax = std::max(1, std::min(16, L[st.l1].cin / 16 / 2));     // a linear bottleneck output may be written as partial slabs (hidden channels split over workgroup groups)
    if (!nv_is_tail(st.kind)) L[st.l1].materialised = true;
    plan->push_back(st);
    i = st.l1 + 1;
  }
  // nv_xblock_kernel, nv_tail_kernel and the pixel-pair kernels of some input widths read ONE input slab, a generic per-layer launch one plain tensor:
  // their producer's partial slabs are summed behind it
  for (size_t si = 0; si < plan->size(); ++si) {
    const NvStep* nx = si + 1 < plan->size() ? &(*plan)[si + 1] : nullptr;
    (*plan)[si].one_slab_out = !nx || !nv_fused(nx->kind) || nx->kind == NvKind::XBlock || nv_is_tail(nx->kind) ||
                               (nx->kind == NvKind::PBlock && nv_pblock_single_input(L[nx->l0].cin));
  }
  return -1;
}

// packs and uploads the weights of one plan step (w: the layer list and head handed to d2fe_load_netvlad)
int nv_pack_step(NvNet& net, NvStep& st, const d2fe_netvlad_weights* w) {
  auto up = [](const std::vector<float>& v, float** dst) { return upload(v.data(), v.size() * sizeof(float), reinterpret_cast<void**>(dst)); };
  const NvKind k = st.kind;
  if (!nv_fused(k)) {
    const d2fe_nv_layer& L = w->layers[st.l0];
    NvLayer& l = net.layers[st.l0];
    std::vector<float> wt, bt;
    if (k == NvKind::Conv0) {
      wt.assign(9 * 32, 0.f); bt.assign(32, 0.f);
      for (int co = 0; co < L.cout; ++co) { bt[co] = L.bias[co]; for (int t = 0; t < 9; ++t) wt[t * 32 + co] = L.weight[co * 9 + t]; }
    } else if (k == NvKind::Dw) {
      wt.resize(9 * (size_t)L.cin); bt.assign(L.bias, L.bias + L.cin);
      for (int c = 0; c < L.cin; ++c) for (int t = 0; t < 9; ++t) wt[(size_t)t * L.cin + c] = L.weight[c * 9 + t];
    } else {
      wt.resize(packed_weight_floats_f32(l.cout_pad, L.cin, 1)); bt.assign(l.cout_pad, 0.f);
      pack_weights_f32(L.weight, L.cout, L.cin, 1, l.cout_pad, wt.data());
      for (int co = 0; co < L.cout; ++co) bt[co] = L.bias[co];
    }
    const int rc = up(wt, &l.w);
    return rc ? rc : up(bt, &l.b);
  }
  const bool front = k == NvKind::Front || k == NvKind::FPair, tail = nv_is_tail(k), pair = k == NvKind::PBlock || k == NvKind::FPair;
  if (front) {
    std::vector<float> pk(384);
    pack_nv_conv0(w->layers[st.l0].weight, w->layers[st.l0].bias, w->layers[st.l0].cout, pk.data());
    const int rc = up(pk, &st.w0);
    if (rc) return rc;
  }
  if (k != NvKind::Block && !front) {       // expand record
    const d2fe_nv_layer& E = w->layers[st.l0];
    std::vector<float> pk;
    switch (k) {
      case NvKind::Tail: pk.resize(pack_nv_expand_floats(E.cout, E.cin)); pack_nv_expand_tail(E.weight, E.bias, E.cout, E.cin, pk.data()); break;
      case NvKind::PBlock: pk.resize(pack_nv_expand_pair_floats(E.cout, E.cin)); pack_nv_expand_pair(E.weight, E.bias, E.cout, E.cin, pk.data()); break;
      case NvKind::XBlock: pk.resize(pack_nv_expand_perm_floats(E.cout, E.cin)); pack_nv_expand_perm(E.weight, E.bias, E.cout, E.cin, pk.data()); break;
      default: pk.resize(pack_nv_expand_floats(E.cout, E.cin)); pack_nv_expand(E.weight, E.bias, E.cout, E.cin, pk.data()); break;
    }
    const int rc = up(pk, &st.we);
    if (rc) return rc;
  }
  // depthwise + project record: the block's dw 3x3 and last 1x1, or (tail) no dw and the NetVLAD pre-projection [proj_dim][feat_dim]
  const d2fe_nv_layer* D = tail ? nullptr : &w->layers[st.l1 - 1];
  const float* pwt = tail ? w->pre_w : w->layers[st.l1].weight;
  const float* pbs = tail ? w->pre_b : w->layers[st.l1].bias;
  const int pco = tail ? w->proj_dim : w->layers[st.l1].cout, pci = tail ? w->feat_dim : w->layers[st.l1].cin;
  // pixel-pair kernels: any n-tile count up to 8 per launch, wider outputs as two channel halves (each with its own project record and bias)
  for (int hf = 0, co0 = 0; hf < st.halves; ++hf) {
    const int pc = pair ? nv_pblock_half_cout(pco, hf) : pco, nt = pair ? nv_pblock_ntiles(pc) : nv_block_ntiles(pco);
    std::vector<float> pk(pair ? pack_nv_dwproj_pair_floats(pci, nt) : pack_nv_dwproj_floats(pci, nt)), pb(nt * 16, 0.f);
    switch (k) {
      case NvKind::PBlock: case NvKind::FPair: pack_nv_dwproj_pair(D->weight, D->bias, pwt, pc, pci, nt, pk.data(), co0); break;
      case NvKind::Tail: pack_nv_proj_t(pwt, pco, pci, nt, pk.data()); break;
      case NvKind::XBlock: pack_nv_dwproj_x(D->weight, D->bias, pwt, pco, pci, nt, pk.data()); break;
      default: pack_nv_dwproj(D ? D->weight : nullptr, D ? D->bias : nullptr, pwt, pco, pci, nt, pk.data()); break;
    }
    for (int co = 0; co < pc; ++co) pb[co] = pbs[co0 + co];
    int rc = up(pk, hf ? &st.wp2 : &st.wp);
    rc = rc ? rc : up(pb, hf ? &st.bp2 : &st.bp);
    if (rc) return rc;
    co0 += pc;
  }
  return D2FE_OK;
}

}  // namespace

namespace d2fe {
int run_netvlad(d2fe_context* h, const uint8_t* d_gray, int n, int W, int H, int stride, size_t image_stride, float* d_out,
                hipStream_t s) {
  ProfScope ps(h, D2FE_PROF_NETVLAD, s);
  const NvNet& net = *h->nv_net;
  const NvKnobs& kn = net.knobs;
  NvRun& run = h->nv_run;
  int ch = H, cw = W;
  bool feat_done = false;
  for (size_t si = 0; si < net.plan.size(); ++si) {
    const NvStep& st = net.plan[si];
    const NvKind k = st.kind;
    if (!nv_fused(k)) {
      const auto& l = net.layers[st.l0];
      const float* in = st.l0 ? run.out[st.l0 - 1] : nullptr;
      float* out = run.out[st.l0];
      const int ho = same_out(ch, l.stride), wo = same_out(cw, l.stride);
      if (k == NvKind::Conv0) HIP_TRY(launch_nv_conv0(d_gray, stride, (long)image_stride, ch, cw, ho, wo, l.stride, l.cout, l.act, l.w, l.b, out, n, s));
      else if (k == NvKind::Dw) HIP_TRY(launch_nv_dw(in, ch, cw, l.cin, ho, wo, l.stride, l.act, l.w, l.b, out, n, s));
      else HIP_TRY(launch_nv_pw(in, (long)n * ch * cw, l.cin, l.cout, l.cout_pad, l.act, l.w, l.b, l.res >= 0 ? run.out[l.res] : nullptr, out, s));
      run.last.layer[st.l0] = NvSlabs();
      ch = ho; cw = wo;
      continue;
    }
    NvBlockArgs a{};
    if (k == NvKind::Front || k == NvKind::FPair) {
      const auto& c0 = net.layers[st.l0];
      a.img = d_gray; a.img_stride = stride; a.img_istride = (long)image_stride; a.H0 = ch; a.W0 = cw;
      const int ho = same_out(ch, c0.stride), wo = same_out(cw, c0.stride);
      a.c0_stride = c0.stride; a.c0_pt = same_pad_begin(ch, c0.stride, ho); a.c0_pl = same_pad_begin(cw, c0.stride, wo);
      a.act0 = c0.act; a.w0 = st.w0;
      ch = ho; cw = wo;
    } else {
      a.in = run.out[st.l0 - 1]; a.in_slabs = run.last.layer[st.l0 - 1].n; a.in_slab_stride = run.last.layer[st.l0 - 1].stride;
    }
    int groups = 1, cpg = 0;
    if (nv_is_tail(k)) {
      // the trunk's last 1x1 (expand: feat_dim hidden channels) chained with the NetVLAD pre-projection, over the flat pixel list
      const auto& e = net.layers[st.l0];
      a.we = st.we; a.act_e = e.act;
      a.H = ch; a.W = cw; a.Ho = ch; a.Wo = cw; a.Cin = e.cin; a.Chid = e.cout; a.Cout = net.proj; a.stride = 1;
      a.P = (long)n * ch * cw;
      a.wp = st.wp; a.bp = st.bp; a.act_p = 0;
      // three workgroups per CU fit (registers), and the MFMA pipe is the limit: ~768 workgroups of equal length load every SIMD alike
      // (the hidden-channel split is decided on ONE image's pixel count whatever the batch: see the block steps below)
      nv_groups(((long)ch * cw + 127) / 128, a.Chid / 16, net.feat_gmax, &groups, &cpg, kn.tail_blocks);
      a.cpg = cpg; a.out = run.feat_buf; a.out_slab_stride = a.P * a.Cout;
      run.last.feat = {groups, a.out_slab_stride, groups};
      if (k == NvKind::Tail) HIP_TRY(launch_nv_tail(a, groups, s));
      else HIP_TRY(launch_nv_block(a, true, 2, n, groups, s));
      // no slab sum here: the VLAD stage reads every feature exactly once and adds the slabs, in slab order, while it stages them
      feat_done = true;
      continue;
    }
    const bool expand = k == NvKind::Expand || k == NvKind::XBlock || k == NvKind::PBlock;
    if (expand) { a.we = st.we; a.act_e = net.layers[st.l0].act; }
    const auto& d = net.layers[st.l1 - 1];
    const auto& pj = net.layers[st.l1];
    a.H = ch; a.W = cw; a.Cin = expand ? net.layers[st.l0].cin : d.cin; a.Chid = d.cin; a.Cout = pj.cout; a.stride = d.stride;
    a.Ho = same_out(ch, d.stride); a.Wo = same_out(cw, d.stride);
    a.pt = same_pad_begin(ch, d.stride, a.Ho); a.pl = same_pad_begin(cw, d.stride, a.Wo);
    a.act_d = d.act;
    a.wp = st.wp; a.bp = st.bp; a.act_p = pj.act;
    if (pj.res >= 0) { a.res = run.out[pj.res]; a.res_slabs = run.last.layer[pj.res].n; a.res_slab_stride = run.last.layer[pj.res].stride; }
    a.th = 8; a.tw = 16;
    if (k == NvKind::PBlock || k == NvKind::FPair) nv_pblock_tile(a.Ho, a.Wo, &a.th, &a.tw, k == NvKind::FPair ? a.c0_stride : 0);
    else if (k == NvKind::XBlock) nv_xblock_tile(a.Ho, a.Wo, a.stride, &a.th, &a.tw);
    const long tiles1 = (long)((a.Wo + a.tw - 1) / a.tw) * ((a.Ho + a.th - 1) / a.th);
    const long tiles = tiles1 * n;
    // partial slabs are summed by the consumer's staging: only when that consumer is a fused step
    // pixel-pair kernel: no more workgroups than 85 % of what the device holds at once (registers / LDS of that block shape).
    // The split of the hidden channels over workgroup groups fixes the fp32 summation order of the block's output, so it is decided on ONE
    // image's tile count and the DEVICE's compute units (not the batch, not a pipeline lane's share): an image's descriptor is the same bits
    // in a 1-image call, a 32-image batch and any pass of the frames-in-flight pipe.  A batch then runs with more groups than it needs to fill
    // the device (15 x 20 layers at 32 images: 7 slabs instead of 4) -- a few MB of partial-slab traffic
    // a consumer that is NOT a fused step (a generic per-layer launch: the stride-2 block 72 -> 432 -> 120 of the 0.75-wide trunk) reads one plain tensor: the split is
    // still worth it (27 chunks in ONE workgroup per tile ran 115 us at 32 images and 70 us for one image; nine groups + the slab sum: 55 + 17 us), the slabs are summed below
    nv_groups(tiles1, a.Chid / 16, pj.gmax, &groups, &cpg, kn.blocks_target,
              (k == NvKind::PBlock || k == NvKind::FPair) ? nv_pblock_slots(a.Cin, a.Cout, h->ncu_dev, 1) * 85 / 100 : 0, st.one_slab_out, kn.group_rule);
    a.cpg = cpg; a.out = run.out[st.l1]; a.out_slab_stride = (long)n * a.Ho * a.Wo * a.Cout;
    // Six or more groups per image (30 x 40 and 15 x 20 layers: what ONE image needs to reach 60-135 workgroups) are 2-3 rounds of short workgroups for a batch, each
    // staging its input patch again and writing its own slab.  The summation order of such a layer is a two-level tree -- runs of `tree` groups, then the runs in order --
    // and a batch lets one workgroup walk a whole run (NvBlockArgs::gmerge): same bits as one image's unmerged launch + tree-ordered slab sum, a third of the
    // workgroups, patch loads and slabs.  `tree` depends on the layer alone, merging on the batch
    int tree = 1, wgroups = groups;
    const int half0 = nv_pblock_half_cout(a.Cout, 0);
    if (k == NvKind::PBlock && groups >= 6 && nv_pblock_can_merge(a.Cin, half0) && (st.halves == 1 || nv_pblock_can_merge(a.Cin, a.Cout - half0))) {
      tree = 3;
      const long slots = nv_pblock_slots(a.Cin, a.Cout, h->ncu_dev, 1);
      if (kn.merge && tiles * groups > slots && tiles * ((groups + tree - 1) / tree) * 2 >= (h->ncu_dev > 0 ? h->ncu_dev : 256)) { a.gmerge = tree; wgroups = (groups + tree - 1) / tree; }
    }
    NvSlabs& slabs = run.last.layer[st.l1];
    slabs = {wgroups, a.out_slab_stride, groups};
    a.ncu = h->ncu; a.tpw = kn.front_tpw; a.nbuf = kn.nbuf;
    if ((int)si == kn.stamp_step && run.stamps && (tiles * wgroups <= 32768)) {
      HIP_TRY(hipMemsetAsync(run.stamps, 0, sizeof(unsigned long long) * 32 * 32768, s));
      a.stamps = run.stamps; run.last.stamp_wgs = (int)(tiles * wgroups);
    }
    switch (k) {
      case NvKind::FPair: HIP_TRY(launch_nv_fpair(a, n, s)); break;
      case NvKind::PBlock: {
        // more than 128 output channels: two launches over channel halves, each with its own project record (the expand + depthwise stages run in both)
        NvBlockArgs h1 = a;
        if (st.halves == 2) { a.co0 = 0; a.Cv = half0; h1.co0 = half0; h1.Cv = a.Cout - half0; h1.wp = st.wp2; h1.bp = st.bp2; h1.stamps = nullptr; }
        HIP_TRY(launch_nv_pblock(a, n, groups, s));
        if (st.halves == 2) HIP_TRY(launch_nv_pblock(h1, n, groups, s));
        break;
      }
      case NvKind::XBlock: HIP_TRY(launch_nv_xblock(a, n, groups, s)); break;
      case NvKind::Front: HIP_TRY(launch_nv_block(a, false, 1, n, groups, s)); break;
      case NvKind::Expand: HIP_TRY(launch_nv_block(a, true, 0, n, groups, s)); break;
      default: HIP_TRY(launch_nv_block(a, false, 0, n, groups, s)); break;       // Block
    }
    // three or more partial slabs: sum them once instead of in every consumer workgroup (and in every residual read)
    // (decided on `groups`, the layer's own count: a consumer sees one slab or several whatever the batch merged)
    // (a tree-ordered layer is always summed here: a consumer adding the slabs itself would do so in slab order, i.e. differently for merged and unmerged launches)
    if (tree > 1 || (kn.slabsum > 0 && groups >= kn.slabsum) || (st.one_slab_out && groups > 1)) {
      HIP_TRY(launch_nv_slab_sum(a.out, wgroups, slabs.stride, slabs.stride, s, a.gmerge > 1 ? 1 : tree));
      slabs.n = 1;
    }
    ch = a.Ho; cw = a.Wo;
  }
  const int np = ch * cw;
  if (!feat_done) {
    const int pp = (net.proj + 31) / 32 * 32;
    HIP_TRY(launch_nv_pw(run.out.back(), (long)n * np, net.feat, net.proj, pp, 0, net.pre_w, net.pre_b, nullptr, run.feat_buf, s));
    run.last.feat = NvSlabs();
  }
  float* raw = net.pca_m ? run.raw : d_out;
  HIP_TRY(launch_nv_vlad(run.feat_buf, run.last.feat.n, run.last.feat.stride, np, net.proj, net.k, net.aw, net.aw_pack, net.ab, net.cen, run.part, raw, n, s));
  if (net.pca_m) HIP_TRY(launch_nv_pca(raw, net.k * net.proj, net.pca_comp, net.pca_mean, net.pca_m, d_out, n, s));
  return D2FE_OK;
}

int nv_check(d2fe_context* h, int n, int W, int H, int stride) {
  if (!h) return fail(D2FE_ERR_INVALID, "null handle");
  if (!h->nv_net) return fail(D2FE_ERR_NOT_READY, "netvlad weights not loaded");
  if (n < 1 || n > h->cfg.max_batch) return fail(D2FE_ERR_INVALID, "batch size out of range");
  if (W < 32 || H < 32 || W > h->cfg.max_width || H > h->cfg.max_height) return fail(D2FE_ERR_INVALID, "image size out of range");
  if (stride < W) return fail(D2FE_ERR_INVALID, "stride < width");
  return D2FE_OK;
}
}  // namespace d2fe

extern "C" {

int d2fe_load_netvlad(d2fe_handle h, const d2fe_netvlad_weights* w) {
  if (h && h->life.pipes() > 0) return fail(D2FE_ERR_INVALID, "the handle has live pipes whose lanes read its packed weights: destroy them before loading weights or PCA matrices");
  if (h) graphs_clear(h);
  if (!h || !w || !w->layers || w->n_layers < 1) return fail(D2FE_ERR_INVALID, "null argument");
  if (!w->pre_w || !w->pre_b || !w->assign_w || !w->assign_b || !w->centroids) return fail(D2FE_ERR_INVALID, "null head weights");
  if (w->n_clusters < 1 || w->n_clusters > 64 || w->proj_dim < 4 || w->proj_dim > 256 || (w->proj_dim & 3) ||
      w->n_clusters * w->proj_dim > 8192 || (w->feat_dim & 3))
    return fail(D2FE_ERR_INVALID, "unsupported NetVLAD head shape");
  HIP_TRY(hipSetDevice(h->cfg.device_id));
  HIP_TRY(hipStreamSynchronize(h->stream));
  // the handle has no network from here on until the new one is complete; a reload keeps the PCA matrices d2fe_set_netvlad_pca left
  auto net = std::make_shared<NvNet>();
  if (h->nv_net) { std::swap(net->pca_comp, h->nv_net->pca_comp); std::swap(net->pca_mean, h->nv_net->pca_mean); std::swap(net->pca_m, h->nv_net->pca_m); }
  h->nv_run.release();
  h->nv_net.reset();
  int rc = nv_describe(w->layers, w->n_layers, h->cfg.max_height, h->cfg.max_width, true, &net->layers);
  if (rc) return rc;
  const int bad = nv_plan(net->layers, w->proj_dim, net->knobs, &net->plan);
  if (bad >= 0) return fail(D2FE_ERR_UNSUPPORTED, "netvlad layer " + std::to_string(bad) + ": residual source is internal to a fused block");
  if (net->layers.back().cout != w->feat_dim) return fail(D2FE_ERR_INVALID, "feat_dim does not match the last layer");
  if (w->feat_dim & 7) return fail(D2FE_ERR_INVALID, "feat_dim must be a multiple of 8");
  net->feat = w->feat_dim; net->proj = w->proj_dim; net->k = w->n_clusters;
  if (nv_is_tail(net->plan.back().kind)) net->feat_gmax = std::max(1, std::min(16, w->feat_dim / 32));
  for (auto& st : net->plan) {       // any failure below frees what was uploaded so far with `net`
    rc = nv_pack_step(*net, st, w);
    if (rc) return rc;
  }
  const int pp = (w->proj_dim + 31) / 32 * 32;
  std::vector<float> pw(packed_weight_floats_f32(pp, w->feat_dim, 1)), pb(pp, 0.f);
  pack_weights_f32(w->pre_w, w->proj_dim, w->feat_dim, 1, pp, pw.data());
  for (int co = 0; co < w->proj_dim; ++co) pb[co] = w->pre_b[co];
  rc = upload(pw.data(), pw.size() * sizeof(float), reinterpret_cast<void**>(&net->pre_w));
  rc = rc ? rc : upload(pb.data(), pb.size() * sizeof(float), reinterpret_cast<void**>(&net->pre_b));
  rc = rc ? rc : upload(w->assign_w, sizeof(float) * w->n_clusters * w->proj_dim, reinterpret_cast<void**>(&net->aw));
  if (w->n_clusters % 16 == 0 && w->proj_dim % 4 == 0) {
    std::vector<float> ap((size_t)w->n_clusters * w->proj_dim);
    pack_nv_assign(w->assign_w, w->n_clusters, w->proj_dim, ap.data());
    rc = rc ? rc : upload(ap.data(), ap.size() * sizeof(float), reinterpret_cast<void**>(&net->aw_pack));
  }
  rc = rc ? rc : upload(w->assign_b, sizeof(float) * w->n_clusters, reinterpret_cast<void**>(&net->ab));
  rc = rc ? rc : upload(w->centroids, sizeof(float) * w->n_clusters * w->proj_dim, reinterpret_cast<void**>(&net->cen));
  if (rc) return rc;
  rc = [&]() -> int {
    const int B = h->cfg.max_batch;
    const int r = h->nv_run.alloc(*net, B);
    if (r) return r;
    if (net->knobs.stamp_step >= 0) HIP_TRY(hipMalloc(&h->nv_run.stamps, sizeof(unsigned long long) * 32 * 32768));
    HostStage& stg = *h->stage;
    if (!stg.nv_s_img) HIP_TRY(stg.dev(&stg.nv_s_img, (size_t)h->cfg.max_width * h->cfg.max_height * B));
    if (!stg.nv_s_out) HIP_TRY(stg.dev(&stg.nv_s_out, sizeof(float) * 8192 * B));
    return D2FE_OK;
  }();
  if (rc) { h->nv_run.release(); return rc; }
  h->nv_net = std::move(net);
  return D2FE_OK;
}

#ifdef D2FE_DEVTOOLS      /* development library only: include/d2fe_debug.h */
/* diagnostics: with D2FE_NV_STAMP_STEP=<plan step> set at d2fe_load_netvlad() time, the wall_clock64() phase stamps [workgroup][32] that step's
 * nv_xblock_kernel wrote during the last d2fe_netvlad* call; returns the number of workgroups (tools/nv_stamps.py). */
long d2fe_debug_netvlad_stamps(d2fe_handle h, unsigned long long* dst, long max_wgs) {
  if (!h || !dst || !h->nv_run.stamps) return fail(D2FE_ERR_NOT_READY, "D2FE_NV_STAMP_STEP was not set when the network was loaded");
  hipSetDevice(h->cfg.device_id);
  const long nw = std::min<long>(max_wgs, h->nv_run.last.stamp_wgs);
  if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(dst, h->nv_run.stamps, sizeof(unsigned long long) * 32 * nw, hipMemcpyDeviceToHost) != hipSuccess)
    return fail(D2FE_ERR_HIP, "D2H");
  return nw;
}

/* test hook: the output of layer `layer` of the loaded network for the last d2fe_netvlad* call (NHWC fp32), if the execution plan
 * materialises it (the last layer of every fused block and every unfused layer); D2FE_ERR_NOT_READY otherwise. */
long d2fe_debug_netvlad_layer(d2fe_handle h, int layer, int n_images, void* dst, size_t max_bytes) {
  if (!h || !dst || !h->nv_net || layer < 0 || layer >= (int)h->nv_net->layers.size() || n_images < 1 || n_images > h->cfg.max_batch)
    return fail(D2FE_ERR_INVALID, "bad argument");
  const auto& l = h->nv_net->layers[layer];
  const float* out = h->nv_run.out[layer];
  const NvSlabs sl = h->nv_run.last.layer[layer];
  if (!out) return fail(D2FE_ERR_NOT_READY, "layer output lives inside a fused block");
  // spatial size of the LAST call: the plan works for any size up to the maximum; the caller passes images of the handle's maximum size here
  const size_t bytes = sizeof(float) * (size_t)n_images * l.oh * l.ow * l.cout;
  if (bytes > max_bytes) return fail(D2FE_ERR_TRUNCATED, "destination too small");
  hipSetDevice(h->cfg.device_id);
  if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(dst, out, bytes, hipMemcpyDeviceToHost) != hipSuccess) return fail(D2FE_ERR_HIP, "D2H");
  if (sl.n > 1) {      // hidden-channel groups wrote partial slabs: the tensor is their sum (what the consumer's staging forms)
    if ((size_t)sl.stride * sizeof(float) != bytes) return fail(D2FE_ERR_INVALID, "n_images differs from the last call");
    std::vector<float> tmp(bytes / sizeof(float));
    float* o = static_cast<float*>(dst);
    for (int s = 1; s < sl.n; ++s) {
      if (hipMemcpy(tmp.data(), out + (size_t)s * sl.stride, bytes, hipMemcpyDeviceToHost) != hipSuccess) return fail(D2FE_ERR_HIP, "D2H");
      for (size_t i = 0; i < tmp.size(); ++i) o[i] += tmp[i];
    }
  }
  return (long)bytes;
}

/* test hook: the pre-projected features [n_images][np][proj_dim] of the last d2fe_netvlad* call (the input of the VLAD stage), partial slabs added in
 * slab order as that stage adds them; the caller passes images of the handle's maximum size, as for d2fe_debug_netvlad_layer. */
long d2fe_debug_netvlad_features(d2fe_handle h, int n_images, void* dst, size_t max_bytes) {
  if (!h || !dst || !h->nv_net || !h->nv_run.feat_buf || n_images < 1 || n_images > h->cfg.max_batch) return fail(D2FE_ERR_INVALID, "bad argument");
  const auto& l = h->nv_net->layers.back();
  const float* feat = h->nv_run.feat_buf;
  const NvSlabs sl = h->nv_run.last.feat;
  const size_t bytes = sizeof(float) * (size_t)n_images * l.oh * l.ow * h->nv_net->proj;
  if (bytes > max_bytes) return fail(D2FE_ERR_TRUNCATED, "destination too small");
  if (sl.n > 1 && (size_t)sl.stride * sizeof(float) != bytes) return fail(D2FE_ERR_INVALID, "n_images differs from the last call");
  hipSetDevice(h->cfg.device_id);
  if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(dst, feat, bytes, hipMemcpyDeviceToHost) != hipSuccess) return fail(D2FE_ERR_HIP, "D2H");
  if (sl.n > 1) {
    std::vector<float> tmp(bytes / sizeof(float));
    float* o = static_cast<float*>(dst);
    for (int s = 1; s < sl.n; ++s) {
      if (hipMemcpy(tmp.data(), feat + (size_t)s * sl.stride, bytes, hipMemcpyDeviceToHost) != hipSuccess) return fail(D2FE_ERR_HIP, "D2H");
      for (size_t i = 0; i < tmp.size(); ++i) o[i] += tmp[i];
    }
  }
  return (long)bytes;
}

/* test hook: how the last d2fe_netvlad* call wrote layer `layer` (-1: the pre-projected features): out[0] = hidden-channel groups of the step that wrote it,
 * out[1] = partial slabs left in memory (1 once the slab-sum launch ran, or for a merged launch's running total) */
int d2fe_debug_netvlad_groups(d2fe_handle h, int layer, int* out) {
  if (!h || !out || !h->nv_net || !h->nv_run.feat_buf || layer < -1 || layer >= (int)h->nv_net->layers.size()) return fail(D2FE_ERR_INVALID, "bad argument");
  const NvSlabs sl = layer < 0 ? h->nv_run.last.feat : h->nv_run.last.layer[layer];
  out[0] = sl.groups; out[1] = sl.n;
  return D2FE_OK;
}

/* test hook: the execution plan d2fe_load_netvlad would build for this layer list and proj_dim under the D2FE_NV_* switches of the environment
 * (weights may be null); needs no GPU.  Writes (kind, first layer, last layer, halves) per step, at most max_steps, and returns the number of steps. */
int d2fe_debug_netvlad_plan(const d2fe_nv_layer* layers, int n_layers, int proj_dim, int* out, int max_steps) {
  if (!layers || n_layers < 1 || (max_steps > 0 && !out)) return fail(D2FE_ERR_INVALID, "bad argument");
  std::vector<NvLayer> L;
  std::vector<NvStep> plan;
  const int rc = nv_describe(layers, n_layers, 480, 640, false, &L);      // (the plan does not depend on the image size)
  if (rc) return rc;
  const int bad = nv_plan(L, proj_dim, NvKnobs(), &plan);
  if (bad >= 0) return fail(D2FE_ERR_UNSUPPORTED, "netvlad layer " + std::to_string(bad) + ": residual source is internal to a fused block");
  for (int i = 0; i < (int)plan.size() && i < max_steps; ++i) {
    const int v[4] = {(int)plan[i].kind, plan[i].l0, plan[i].l1, plan[i].halves};
    memcpy(out + 4 * i, v, sizeof(v));
  }
  return (int)plan.size();
}
#endif  // D2FE_DEVTOOLS

int d2fe_set_netvlad_pca(d2fe_handle h, const float* comp, const float* mean, int m) {
  if (h && h->life.pipes() > 0) return fail(D2FE_ERR_INVALID, "the handle has live pipes whose lanes read its packed weights: destroy them before loading weights or PCA matrices");
  if (h) graphs_clear(h);
  if (!h) return fail(D2FE_ERR_INVALID, "null handle");
  if (!h->nv_net) return fail(D2FE_ERR_NOT_READY, "netvlad weights not loaded");
  NvNet& net = *h->nv_net;
  const int G = net.k * net.proj;
  if (m < 0 || m > 8192 || (m > 0 && (!comp || !mean)) || (G & 3)) return fail(D2FE_ERR_INVALID, "bad PCA arguments");
  HIP_TRY(hipSetDevice(h->cfg.device_id));
  HIP_TRY(hipStreamSynchronize(h->stream));
  if (net.pca_comp) { hipFree(net.pca_comp); net.pca_comp = nullptr; }
  if (net.pca_mean) { hipFree(net.pca_mean); net.pca_mean = nullptr; }
  net.pca_m = 0;
  if (m == 0) return D2FE_OK;
  int rc = upload(comp, sizeof(float) * (size_t)m * G, reinterpret_cast<void**>(&net.pca_comp));
  rc = rc ? rc : upload(mean, sizeof(float) * G, reinterpret_cast<void**>(&net.pca_mean));
  if (rc) return rc;
  net.pca_m = m;
  return D2FE_OK;
}

int d2fe_netvlad_dim(d2fe_handle h) {
  if (!h || !h->nv_net) return fail(D2FE_ERR_NOT_READY, "netvlad weights not loaded");
  return h->nv_net->pca_m ? h->nv_net->pca_m : h->nv_net->k * h->nv_net->proj;
}

int d2fe_netvlad_device(d2fe_handle h, const uint8_t* d_gray, int n, int width, int height, int stride, size_t image_stride,
                        float* d_out, void* stream) {
  int rc = nv_check(h, n, width, height, stride);
  if (rc) return rc;
  if (!d_gray || !d_out) return fail(D2FE_ERR_INVALID, "null device pointer");
  HIP_TRY(hipSetDevice(h->cfg.device_id));
  return run_netvlad(h, d_gray, n, width, height, stride, image_stride, d_out, stream ? (hipStream_t)stream : h->stream);
}

int d2fe_netvlad_batch(d2fe_handle h, const uint8_t* gray, int n, int width, int height, int stride, size_t image_stride,
                       float* out) {
  int rc = nv_check(h, n, width, height, stride);
  if (rc) return rc;
  if (!gray || !out) return fail(D2FE_ERR_INVALID, "null pointer");
  HIP_TRY(hipSetDevice(h->cfg.device_id));
  hipStream_t s = h->stream;
  HostStage& stg = *h->stage;
  rc = upload_frames(h, stg.nv_s_img, gray, n, width, height, stride, image_stride, s);
  if (rc) return rc;
  rc = run_cached(h, {2, n, width, height, (long)h->nv_net->pca_m, 0}, s, [&](hipStream_t st) {
    return run_netvlad(h, stg.nv_s_img, n, width, height, width, (size_t)width * height, stg.nv_s_out, st);
  });
  if (rc) return rc;
  const int G = d2fe_netvlad_dim(h);
  const size_t bytes = sizeof(float) * (size_t)G * n;
  const bool pinned = h->use_pinned && stg.pin_out && bytes <= stg.pin_out_bytes;      // one D2H into the pinned staging, or straight into `out`
  HIP_TRY(hipMemcpyAsync(pinned ? (void*)stg.pin_out : (void*)out, stg.nv_s_out, bytes, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (pinned) memcpy(out, stg.pin_out, bytes);
  return D2FE_OK;
}

int d2fe_netvlad(d2fe_handle h, const uint8_t* gray, int width, int height, int stride, float* out) {
  return d2fe_netvlad_batch(h, gray, 1, width, height, stride, (size_t)stride * height, out);
}

}  // extern "C"
