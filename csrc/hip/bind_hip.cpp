// pybind11 module `_onihip`: thin launch bindings for the gfx950 kernels.
//
// Arguments are raw device addresses (torch tensor .data_ptr()) and the HIP
// stream handle of the caller (torch.cuda.current_stream().cuda_stream), so
// launches join torch's stream order and can be captured into hipGraphs.
// Shape/dtype/contiguity validation happens in oni_ml_amd/ops/hip.py before
// any launch.
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <stdexcept>
#include <tuple>
#include <string>
#include <vector>

#include "common.h"
#include "kernels.h"

namespace py = pybind11;
using u = uintptr_t;

template <typename T>
static T* P(u x) {
  return reinterpret_cast<T*>(x);
}
static hipStream_t S(u x) { return reinterpret_cast<hipStream_t>(x); }

PYBIND11_MODULE(_onihip, m) {
  m.doc() = "oni_ml_amd CDNA4 (gfx950) HIP kernels";

  m.def("compiled_ks", []() {
    std::vector<int> v;
#define ONI_KS(X) v.push_back(X);
    ONI_FOR_EACH_KS(ONI_KS)
#undef ONI_KS
    return v;
  });

  m.def("device_name", []() {
    hipDeviceProp_t p;
    int dev = 0;
    ONI_HIP_CHECK(hipGetDevice(&dev));
    ONI_HIP_CHECK(hipGetDeviceProperties(&p, dev));
    return std::string(p.gcnArchName);
  });

  m.def("suff_fused_blocks", [](int h, int m_, int l) { return oni::suff_fused_blocks(h, m_, l); });
  m.def("rows_accumulate", [](u rows, u ptr, u src, u own, u recv, u out, int n_rows, int width, u stream) {
    oni::launch_rows_accumulate(P<const int>(rows), P<const int>(ptr), P<const int>(src), P<const double>(own),
                                P<const double>(recv), P<double>(out), n_rows, width, S(stream));
  });
  m.def("log_beta_t", [](u cw, int V, int K, int ld, u ct, double floor_v, u out, u stream) {
    oni::launch_log_beta_t(P<const double>(cw), V, K, ld, P<const double>(ct), floor_v, P<double>(out), S(stream));
  });
  m.def("colsum_partials", [](u part, int nb, int cols, u out, u gate, u stream) {
    oni::launch_colsum_partials(P<const double>(part), nb, cols, P<double>(out), P<const double>(gate), S(stream));
  });
  m.def("em_control", [](u scalars, u params, u ctl, u hist, int hist_slots, u stream) {
    oni::launch_em_control(P<const double>(scalars), P<double>(params), P<double>(ctl), P<double>(hist), hist_slots,
                           S(stream));
  });
  m.def("param_count", []() { return oni::kParamCount; });
  m.def("hist_cols", []() { return oni::kHistCols; });

  m.def("alpha_newton", [](u scalars, double num_docs, int K, bool estimate, u params, u alpha_out, u stream) {
    oni::launch_alpha_newton(P<const double>(scalars), num_docs, K, estimate, P<double>(params), P<double>(alpha_out),
                             S(stream));
  });


  // ---------------------------------------------- fp64 block Gauss-Seidel ---
  m.def("gs_umax", [](int KS) { return KS > 0 ? oni::gs_umax(KS) : oni::kGsUMax; }, py::arg("KS") = 0);
  m.def("gs_tiny_max", [](int KS) { return oni::gs_tiny_max(KS); });
  m.def("gs_estep", [](u doc_ptr, u word_idx, u counts, u order, int n_items, u beta, int K, int KS, int gs_updates,
                       u params, u gamma, u cphi, u lik, u alpha_ss, u iters, int variant, u stream, u dbg,
                       u stage, u stage_off, u csum, u et) {
    oni::GSArgs a{P<const int>(doc_ptr), P<const int>(word_idx), P<const float>(counts), P<const int>(order),
                  n_items,               P<const double>(beta),  K,                      gs_updates,
                  P<const double>(params), P<double>(gamma),     P<double>(cphi),        P<double>(lik),
                  P<double>(alpha_ss),   P<int>(iters),         P<long long>(dbg),      P<const double>(stage),
                  P<const long long>(stage_off), P<const double>(csum), P<double>(et)};
    oni::launch_gs_estep(a, variant, KS, S(stream));
  }, py::arg("doc_ptr"), py::arg("word_idx"), py::arg("counts"), py::arg("order"), py::arg("n_items"),
     py::arg("beta"), py::arg("K"), py::arg("KS"), py::arg("gs_updates"), py::arg("params"), py::arg("gamma"),
     py::arg("cphi"), py::arg("lik"), py::arg("alpha_ss"), py::arg("iters"), py::arg("variant"), py::arg("stream"),
     py::arg("dbg"), py::arg("stage"), py::arg("stage_off"), py::arg("csum") = (u)0, py::arg("et") = (u)0);
  m.def("gs_stage", [](u beta, u word_idx, u tile_ent, u tile_cnt, int n_tiles, u stage, int KS, u gate, u stream) {
    oni::launch_gs_stage(P<const double>(beta), P<const int>(word_idx), P<const int>(tile_ent),
                         P<const int>(tile_cnt), n_tiles, P<double>(stage), KS, P<const double>(gate), S(stream));
  });
  m.def("init_random_ss", [](u cw, int V, int K, int KS, unsigned long long seed, u stream) {
    oni::launch_init_random_ss(P<double>(cw), V, K, KS, seed, S(stream));
  });
  m.def("gs_split_capacity", [](int KS) { return oni::gs_split_capacity(KS); });
  m.def("gs_split_umax", [](int KS) { return oni::gs_split_umax(KS); });
  m.def("gs_split_lds_umax", [](int KS) { return oni::gs_split_lds_umax(KS); });
  m.def("gs_split", [](u doc_ptr, u word_idx, u counts, u beta, int K, int KS, int gs_updates, u params, u gamma,
                       u cphi, u lik, u alpha_ss, u iters, u seg_doc, u seg_index, u seg_count, u seg_base,
                       u doc_slot, int n_blocks, u xchg, u counter, int n_docs, u error, u stream, u dbg, u tab,
                       int tab_rows, u csum, int csum_stride) {
    oni::GSArgs a{P<const int>(doc_ptr), P<const int>(word_idx), P<const float>(counts), nullptr,
                  n_blocks,              P<const double>(beta),  K,                      gs_updates,
                  P<const double>(params), P<double>(gamma),     P<double>(cphi),        P<double>(lik),
                  P<double>(alpha_ss),   P<int>(iters),         P<long long>(dbg)};
    oni::SplitArgs s{P<const int>(seg_doc), P<const int>(seg_index), P<const int>(seg_count),
                     P<const int>(seg_base), P<const int>(doc_slot), n_blocks, tab_rows,
                     P<unsigned long long>(xchg), P<int>(counter), n_docs, P<int>(error), P<double>(tab),
                     P<const double>(csum), csum_stride};
    oni::launch_gs_split(a, s, KS, S(stream));
  });
  m.def("gs_suff64", [](u word_ptr, u csc_ent, u order, int n_heavy, int n_medium, int n_light, u cphi, u cw, u part,
                        u lik, u ass, int lo, int hi, int KS, u gate, u stream, u cw_base, u rc_beta, u rc_et,
                        u rc_et_row, u rc_counts) {
    const oni::SuffRecompArgs rc{P<const double>(rc_beta), P<const double>(rc_et), P<const int>(rc_et_row),
                                 P<const float>(rc_counts)};
    oni::launch_gs_suff64(P<const int>(word_ptr), P<const int>(csc_ent), P<const int>(order), n_heavy, n_medium,
                          n_light, P<const double>(cphi), P<double>(cw), P<double>(part), P<const double>(lik),
                          P<const double>(ass), lo, hi, KS, P<const double>(gate), S(stream),
                          P<const double>(cw_base), rc);
  }, py::arg("word_ptr"), py::arg("csc_ent"), py::arg("order"), py::arg("n_heavy"), py::arg("n_medium"),
     py::arg("n_light"), py::arg("cphi"), py::arg("cw"), py::arg("part"), py::arg("lik"), py::arg("ass"),
     py::arg("lo"), py::arg("hi"), py::arg("KS"), py::arg("gate"), py::arg("stream"), py::arg("cw_base"),
     py::arg("rc_beta") = (u)0, py::arg("rc_et") = (u)0, py::arg("rc_et_row") = (u)0, py::arg("rc_counts") = (u)0);
  m.def("gs_mstep_control", [](u cw, u class_total, u beta, int V, int K, int KS, u scalars, u params, u ctl,
                               u hist, int hist_slots, u done_count, u stream, u rows, int n_rows, int newton,
                               int estimate, double num_docs, u alpha_out, u st_word_idx,
                               std::vector<std::tuple<u, u, u, int>> st_sets) {
    oni::EMControlArgs c{P<const double>(scalars), P<double>(params), P<double>(ctl), P<double>(hist), hist_slots,
                         P<int>(done_count)};
    const oni::NewtonArgs nw{newton, estimate, num_docs, P<double>(alpha_out)};
    if (newton && !alpha_out) throw std::runtime_error("gs_mstep_control: alpha_out required with newton");
    oni::StageFuseArgs sf;
    if (st_sets.size() > 2) throw std::runtime_error("gs_mstep_control: at most 2 staged sets");
    sf.word_idx = P<const int>(st_word_idx);
    for (const auto& [ent, cnt, out, n] : st_sets) {
      sf.tile_ent[sf.n_sets] = P<const int>(ent);
      sf.tile_cnt[sf.n_sets] = P<const int>(cnt);
      sf.out[sf.n_sets] = P<double>(out);
      sf.n_tiles[sf.n_sets] = n;
      ++sf.n_sets;
    }
    oni::launch_gs_mstep_control(P<const double>(cw), P<const double>(class_total), P<double>(beta), V, K, KS,
                                 P<const int>(rows), n_rows, c, nw, S(stream), sf);
  }, py::arg("cw"), py::arg("class_total"), py::arg("beta"), py::arg("V"), py::arg("K"), py::arg("KS"),
     py::arg("scalars"), py::arg("params"), py::arg("ctl"), py::arg("hist"), py::arg("hist_slots"),
     py::arg("done_count"), py::arg("stream"), py::arg("rows"), py::arg("n_rows"), py::arg("newton"),
     py::arg("estimate"), py::arg("num_docs"), py::arg("alpha_out"), py::arg("st_word_idx") = 0,
     py::arg("st_sets") = std::vector<std::tuple<u, u, u, int>>());
  m.def("gs_mstep", [](u cw, u class_total, u beta, int V, int K, int KS, u gate, u stream) {
    oni::launch_gs_mstep(P<const double>(cw), P<const double>(class_total), P<double>(beta), V, K, KS,
                         P<const double>(gate), S(stream));
  });

  m.def("score_events", [](u theta, u phi, int K, double dflt, u doc_a, u word_a, u doc_b, u word_b,
                           int64_t n, double tol, u score_a, u score_b, u key, u flag, u stream) {
    oni::ScoreArgs a{P<const double>(theta), P<const double>(phi), K, dflt,
                     P<const int>(doc_a),    P<const int>(word_a), P<const int>(doc_b),
                     P<const int>(word_b),   n,                    tol,
                     P<double>(score_a),     P<double>(score_b),   P<double>(key),
                     P<uint8_t>(flag)};
    oni::launch_score_events(a, S(stream));
  });

  m.def("ensemble_max", []() { return oni::kEnsembleMax; });
  m.def("score_ensemble", [](u theta, u phi, int R, int K, double dflt, u doc_a, u word_a, u doc_b, u word_b,
                             int64_t n, double tol, u score_a, u score_b, u key, u flag, u votes, int max_blocks,
                             u stream) {
    oni::EnsembleScoreArgs a{P<const double>(theta), P<const double>(phi), R, K, dflt,
                             P<const int>(doc_a),    P<const int>(word_a), P<const int>(doc_b),
                             P<const int>(word_b),   n,                    tol,
                             P<double>(score_a),     P<double>(score_b),   P<double>(key),
                             P<uint8_t>(flag),       P<uint8_t>(votes)};
    oni::launch_score_ensemble(a, max_blocks, S(stream));
  });

  m.def("select_tile", []() { return oni::kSelectTile; });
  m.def("select_work_words", [](int64_t n) { return oni::select_work_words(n); });
  m.def("select_result_word", []() { return oni::select_result_word(); });
  m.def("select_lowest", [](u key, u flag, int64_t n, int64_t limit, u work, u out, int64_t out_cap, int max_blocks,
                            u stream) {
    if (n <= 0 || n >= ((int64_t)1 << 31)) throw std::runtime_error("select_lowest: n outside 1 .. 2^31 - 1");
    if (limit < 1 || limit > n || out_cap < limit) throw std::runtime_error("select_lowest: limit outside 1 .. n");
    oni::SelectArgs a{P<const double>(key), P<const uint8_t>(flag), n, (unsigned)limit,
                      (unsigned)((n + oni::kSelectTile - 1) / oni::kSelectTile), P<unsigned>(work),
                      P<long long>(out), (unsigned)out_cap};
    oni::launch_select_lowest(a, max_blocks, S(stream));
  });

  m.def("host_summary", [](u doc_a, u score_a, u doc_b, u score_b, int64_t n, int64_t D, double tol, u events,
                           u flagged, u min_key, u worst, u skipped, bool fold, u stats, int max_blocks, u stream) {
    if (n <= 0 || n >= ((int64_t)1 << 31) || D <= 0 || D >= ((int64_t)1 << 31))
      throw std::runtime_error("host_summary: n or D outside 1 .. 2^31 - 1");
    oni::HostSummaryArgs a{P<const int>(doc_a), P<const double>(score_a), P<const int>(doc_b),
                           P<const double>(score_b), n, D, tol, P<unsigned>(events), P<unsigned>(flagged),
                           P<unsigned long long>(min_key), P<unsigned>(worst), P<unsigned>(skipped), fold ? 1 : 0,
                           P<unsigned long long>(stats)};
    oni::launch_host_summary(a, max_blocks, S(stream));
  });

  m.def("explain_max_fields", []() { return oni::kExplainMaxFields; });
  m.def("group_rows_sum", [](u table, u order, u seg_start, u seg_end, u blk_off, int64_t G, int64_t B, int W,
                             int block, u scratch, u out, int max_blocks, u stream) {
    oni::GroupRowsArgs a{P<const double>(table),    P<const int>(order),     P<const int64_t>(seg_start),
                         P<const int64_t>(seg_end), P<const int64_t>(blk_off), G, B, W, block,
                         P<double>(scratch),        P<double>(out)};
    oni::launch_group_rows_sum(a, max_blocks, S(stream));
  });
  m.def("explain_sides", [](u theta, u phi, u gsum, int R, int K, int F, double dflt, u doc, u word, u grow,
                            int64_t n, u cond, u why, int max_blocks, u stream) {
    oni::ExplainArgs a{P<const double>(theta), P<const double>(phi), P<const double>(gsum), R, K, F, dflt,
                       P<const int>(doc),      P<const int>(word),   P<const int>(grow),    n,
                       P<double>(cond),        P<uint8_t>(why)};
    oni::launch_explain_sides(a, max_blocks, S(stream));
  });

  m.def("expect_theta_path", [](int R, int K) { return oni::expect_theta_path(R, K); });
  m.def("expect_sides", [](u theta, u phi, int R, int K, double dflt, u order, u doc, u word, u seg_start, u seg_end,
                           u out_at, u blk_off, u blk_item, int64_t n, int64_t B, int block, u part_p, u part_best,
                           u part_above, u best, u pbest, u above, int max_blocks, u stream) {
    oni::ExpectArgs a{P<const double>(theta),      P<const double>(phi),      R, K, dflt,
                      P<const int>(order),         P<const int>(doc),         P<const int>(word),
                      P<const int64_t>(seg_start), P<const int64_t>(seg_end), P<const int64_t>(out_at),
                      P<const int64_t>(blk_off),   P<const int>(blk_item),    n, B, block,
                      P<double>(part_p),           P<int>(part_best),         P<int>(part_above),
                      P<int>(best),                P<double>(pbest),          P<int>(above)};
    oni::launch_expect_sides(a, max_blocks, S(stream));
  });

  m.def("tail_theta_path", [](int R, int K) { return oni::tail_theta_path(R, K); });
  m.def("tail_mass", [](u theta, u phi, int R, int K, int64_t V, u doc, u word, int64_t n, int64_t block,
                        int64_t nblk, u scratch, u le, u tot, u rarer, u ties, int max_blocks, u stream) {
    oni::TailArgs a{P<const double>(theta), P<const double>(phi), R, K, V, P<const int>(doc), P<const int>(word), n,
                    block, nblk, P<double>(scratch), P<double>(le), P<double>(tot), P<int>(rarer), P<int>(ties)};
    oni::launch_tail_mass(a, max_blocks, S(stream));
  });
  m.def("tail_mass_docs", [](u theta, u phi, int R, int K, int64_t V, u doc, u word, int64_t n, int64_t block,
                             int64_t nblk, u scratch, u le, u tot, u rarer, u ties, int max_blocks, u stream) {
    oni::TailArgs a{P<const double>(theta), P<const double>(phi), R, K, V, P<const int>(doc), P<const int>(word), n,
                    block, nblk, P<double>(scratch), P<double>(le), P<double>(tot), P<int>(rarer), P<int>(ties)};
    oni::launch_tail_docs(a, max_blocks, S(stream));
  });

  m.def("peers_max", []() { return oni::kPeersMax; });
  m.def("peer_theta_path", [](int R, int K) { return oni::peer_theta_path(R, K); });
  m.def("peer_topn", [](u theta, int W, int64_t D, u query, int64_t n, int N, int64_t block, int64_t nblk, u scratch,
                        u rows, u dist, u count, int max_blocks, u stream) {
    oni::PeerArgs a{P<const double>(theta), W, D, P<const int>(query), n, N, block, nblk, P<double>(scratch),
                    P<int>(rows), P<double>(dist), P<int>(count)};
    oni::launch_peer_topn(a, max_blocks, S(stream));
  });

  m.def("topic_report_max", []() { return oni::kTopicReportMax; });
  m.def("topic_columns_max", []() { return oni::kTopicColumnsMax; });
  m.def("topic_threads", [](int N) { return oni::topic_threads(N); });
  m.def("topic_merge_groups", [](int64_t nblk) { return oni::topic_merge_groups(nblk); });
  m.def("topic_groups", [](int N, int wb) { return oni::topic_groups(N, wb); });
  m.def("column_topn", [](u table, int64_t rows, int W, int64_t ld, u tau, int c0, int wb, int N, int64_t block,
                          int64_t nblk, u scratch, u scratch2, u out_rows, u out_vals, u out_count, int max_blocks,
                          u stream) {
    oni::TopnArgs a{P<const double>(table), rows, W, ld, P<const double>(tau), c0, wb, N, block, nblk, P<double>(scratch), P<double>(scratch2),
                    P<int>(out_rows), P<double>(out_vals), P<int>(out_count)};
    oni::launch_column_topn(a, max_blocks, S(stream));
  });
  m.def("row_dominant", [](u table, int64_t rows, int R, int K, u arg, u counts, int max_blocks, u stream) {
    oni::DominantArgs a{P<const double>(table), rows, R, K, P<int>(arg), P<unsigned long long>(counts)};
    oni::launch_row_dominant(a, max_blocks, S(stream));
  });
  m.def("topic_sides", [](u theta, u phi, int R, int K, u doc, u word, int64_t n, u col, u resp, u host_share,
                          u host_topic, int max_blocks, u stream) {
    oni::TopicSidesArgs a{P<const double>(theta), P<const double>(phi), R, K, P<const int>(doc), P<const int>(word), n,
                          P<int>(col), P<double>(resp), P<double>(host_share), P<int>(host_topic)};
    oni::launch_topic_sides(a, max_blocks, S(stream));
  });

  m.def("column_l1_width_max", []() { return oni::kColumnL1WidthMax; });
  m.def("column_l1_tile", [](int W) { return oni::column_l1_tile(W); });
  m.def("column_l1", [](u A, u B, int64_t Va, int64_t Vb, int Wa, int Wb, u ia, u ib, int64_t M, int64_t block,
                        int64_t b0, int64_t nb, u scratch, u C, bool first, int max_blocks, u stream) {
    oni::ColumnL1Args a{P<const double>(A), P<const double>(B), Va, Vb, Wa, Wb, P<const int64_t>(ia),
                        P<const int64_t>(ib), M, block, b0, nb, P<double>(scratch), P<double>(C), first ? 1 : 0};
    oni::launch_column_l1(a, max_blocks, S(stream));
  });

  m.def("holdout_draw", [](u base, u counts, u chunk_off, int64_t nnz, int64_t chunks, unsigned long long key,
                           unsigned long long thr, int lane_tokens, u t, int max_blocks, u stream) {
    oni::HoldoutDrawArgs a{P<const int64_t>(base), P<const int64_t>(counts), P<const int64_t>(chunk_off), nnz, chunks,
                           key, thr, lane_tokens, P<int64_t>(t)};
    oni::launch_holdout_draw(a, max_blocks, S(stream));
  });
  m.def("holdout_entries", [](u theta, u phi, int K, u doc, u word, u t, u seen, int64_t n, u ll, int max_blocks,
                              u stream) {
    oni::HoldoutEntriesArgs a{P<const double>(theta), P<const double>(phi), K, P<const int>(doc), P<const int>(word),
                              P<const int64_t>(t), P<const uint8_t>(seen), n, P<double>(ll)};
    oni::launch_holdout_entries(a, max_blocks, S(stream));
  });

  m.def("string_entropy", [](u bytes, u offsets, int64_t n, u table, int64_t table_len, u out, int max_blocks,
                             u stream) {
    if (n < 0 || table_len < 2 || max_blocks < 0) throw std::runtime_error("string_entropy: bad sizes");
    oni::StringEntropyArgs a{P<const uint8_t>(bytes), P<const int64_t>(offsets), n, P<const double>(table),
                             table_len, P<double>(out)};
    oni::launch_string_entropy(a, max_blocks, S(stream));
  });

  m.def("flow_words", [](u hour, u minute, u second, u port_a, u port_b, u ipkt, u ibyt, u time_cuts,
                         int n_time, u ibyt_cuts, int n_ibyt, u ipkt_cuts, int n_ipkt, int64_t n, u time_out,
                         u time_bin, u ibyt_bin, u ipkt_bin, u word_port, u p_case, u src_prefix,
                         u dst_prefix, u stream) {
    oni::FlowWordArgs a{};
    a.hour = P<const double>(hour);
    a.minute = P<const double>(minute);
    a.second = P<const double>(second);
    a.port_a = P<const double>(port_a);
    a.port_b = P<const double>(port_b);
    a.ipkt = P<const double>(ipkt);
    a.ibyt = P<const double>(ibyt);
    a.time_cuts = P<const double>(time_cuts);
    a.ibyt_cuts = P<const double>(ibyt_cuts);
    a.ipkt_cuts = P<const double>(ipkt_cuts);
    a.n_time_cuts = n_time;
    a.n_ibyt_cuts = n_ibyt;
    a.n_ipkt_cuts = n_ipkt;
    a.n = n;
    a.time_out = P<double>(time_out);
    a.time_bin = P<int8_t>(time_bin);
    a.ibyt_bin = P<int8_t>(ibyt_bin);
    a.ipkt_bin = P<int8_t>(ipkt_bin);
    a.word_port = P<double>(word_port);
    a.p_case = P<int8_t>(p_case);
    a.src_prefix = P<int8_t>(src_prefix);
    a.dst_prefix = P<int8_t>(dst_prefix);
    oni::launch_flow_words(a, S(stream));
  });

  m.def("csc_part_tile", []() { return oni::kCscPartTile; });
  m.def("csc_docs", [](u perm, u doc_ptr, int D, int nnz, u csc_ent, u csc_doc, u stream) {
    oni::launch_csc_docs(P<const long long>(perm), P<const int>(doc_ptr), D, nnz, P<int>(csc_ent), P<int>(csc_doc),
                         S(stream));
  });
  m.def("csc_partition", [](u csc_ent, u csc_doc, u word_ptr, u late, int nnz, int V, int D, int n_early, int n_late,
                            u ce_early, u ce_late, u wp_early, u wp_late, u tile_sum, u before, u et_row, u et_s0,
                            u et_w, u et_base, int umax, u stream) {
    oni::CscPartArgs a{P<const int>(csc_ent), P<const int>(csc_doc), P<const int>(word_ptr), P<const uint8_t>(late),
                       nnz, V, D, n_early, n_late, P<int>(ce_early), P<int>(ce_late), P<int>(wp_early),
                       P<int>(wp_late), P<int>(tile_sum), P<int>(before), P<int>(et_row), P<const int>(et_s0),
                       P<const int>(et_w), P<const int>(et_base), umax};
    oni::launch_csc_partition(a, S(stream));
  });

  m.def("bin_columns", [](std::vector<u> values, std::vector<u> cuts, std::vector<int> ncuts, int64_t n,
                          u bins, u stream) {
    if (values.size() != cuts.size() || values.size() != ncuts.size())
      throw std::runtime_error("bin_columns: column lists differ in length");
    std::vector<const double*> v, c;
    for (auto x : values) v.push_back(P<const double>(x));
    for (auto x : cuts) c.push_back(P<const double>(x));
    oni::launch_bin_columns(v.data(), c.data(), ncuts.data(), (int)values.size(), n, P<int8_t>(bins),
                            S(stream));
  });
}
