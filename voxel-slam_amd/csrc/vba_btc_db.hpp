// Private header of the units that read a descriptor database ("Source layout": where state lives): the handle struct of
// vba_btc.hip and the declarations of what that unit defines and the keyframe store calls.  It defines no kernel.
#pragma once
#include "vba_ctx.hpp"
#include "vba_btcgen.hpp"

// loop retrieval (vba_btc.hip); the keyframe store writes the generator's point buffer (db->gen->xyz)
struct vba_btc_db {
  vba_ctx *ctx = nullptr;
  vba_btc_config cfg{};
  int nstd = 0, cap = 0;                     // descriptors stored / capacity (rows)
  BtcStds d{};                               // the view the kernels take of the six arrays below (btc_reserve_rows)
  DevMem<double> tri, cen, loc; DevMem<unsigned long long> bits; DevMem<int> summ, frame;
  std::vector<int> tab;                      // host mirror of the cell table, 8 ints per slot (vba_kernels_btc.hpp)
  int tab_mask = 0, ncell = 0;
  DevMem<int> d_tab;
  int nchunk = 0, chunk_cap = 0;
  DevMem<int> d_ent, d_next;
  std::vector<int> off{0}, seq;              // plane clouds: point offsets, header.seq
  DevMem<float> d_pc; size_t pc_cap = 0;
  DevMem<int> d_off; int off_cap = 0;
  int mcap = 0; DevMem<int> d_m;             // match list and per-candidate pair lists: mq | md | mf | pq | pd, mcap each
  int vcap = 0; DevMem<int> d_votes;
  DevMem<int> d_cand, d_total; DevMem<double> d_cres, d_res; PinMem<double> h_res;
  bool have_search = false;                  // the last search ran the kernels (n > 0)
  // descriptor generation (vba_btc_generate_stds): its configuration, device buffers, the AddSTDescs count (current_frame_id_)
  // and the corners of the last call
  vba_btc_gen_config gcfg{};
  BtcGen *gen = nullptr;
  int n_add = 0;
  std::vector<double> last_loc; std::vector<uint64_t> last_bits;
  BtcCfgDev dev_cfg() const {
    BtcCfgDev f;
    f.skip_near = cfg.skip_near_num; f.cand_num = cfg.candidate_num; f.rough = cfg.rough_dis_threshold; f.sim = cfg.similarity_threshold;
    f.icp = cfg.icp_threshold; f.normal = cfg.normal_threshold; f.dis = cfg.dis_threshold;
    return f;
  }
  BtcIndex index() const { BtcIndex ix; ix.tab = d_tab; ix.mask = tab_mask; ix.ent = d_ent; ix.next = d_next; return ix; }
};

namespace vba {
int btc_gen_ensure(vba_btc_db *db, int64_t points, int64_t cells, size_t corners);
int btc_generate_check(vba_btc_db *db, int n, int cap, double *rows, uint64_t *bits, int *n_stds);
int btc_generate_impl(vba_btc_db *db, int n, const float *xyz, int id, int cap, double *rows, uint64_t *bits, int *n_stds);
}  // namespace vba
