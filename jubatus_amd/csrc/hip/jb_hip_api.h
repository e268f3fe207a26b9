// The C ABI of libjubatus_hip.so: the one declaration of every exported
// jb_* function. Every .hip file that defines or calls one includes this
// header, so a definition that drifts from it is a compile error; the native
// servers (csrc/server) include it instead of copying prototypes, and
// tests/test_hip_abi.py checks the ctypes table of ops/hip.py against it by
// type. Host declarations only: nothing here needs a device compiler.
#ifndef JUBATUS_AMD_CSRC_HIP_JB_HIP_API_H_
#define JUBATUS_AMD_CSRC_HIP_JB_HIP_API_H_
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "jb_train_batch.hpp"

extern "C" {

// classify_direct.hip
int jb_classify_direct(const int32_t* idx, const float* val, const int64_t* row_ptr, int n,
                       const float* W, int LC, float* out_host, uint32_t* done_host,
                       hipStream_t stream);
int jb_classify_direct_bf16(const int32_t* idx, const float* val, const int64_t* row_ptr, int n,
                            const uint16_t* W, int LC, float* out_host, uint32_t* done_host,
                            hipStream_t stream);
int jb_diag_empty(uint32_t* done_host, int spin, hipStream_t stream);
void* jb_host_alloc(int64_t nbytes);
int jb_host_free(void* p);

// clustering.hip
int jb_gmm_em(const float* X, int n, int d, const float* w, float* C, float* var, float* pi, int k,
              int iters, int32_t* assign, hipStream_t stream);
int jb_argmin_rows(const float* D, int64_t n, int k, int32_t* out, hipStream_t stream);
int jb_sqdist_mfma(const float* X, int64_t n, const float* C, int k, int d, const float* xn2,
                   const float* cn2, float* out, hipStream_t stream);
int jb_kmeanspp(const float* X, int n, int d, const float* w, const double* u, int m, float* d2,
                float* prob, int32_t* out, int32_t* status, hipStream_t stream);
int jb_lloyd(const float* X, int n, int d, const float* w, float* C, int k, int iters, float atol,
             float rtol, int32_t* assign, float* S, int32_t* done_iters, hipStream_t stream);

// dbscan.hip
int jb_dbscan(const float* X, int n, int d, const float* xn2, const float* w, float eps2,
              float min_mass, uint64_t* adj, float* mass, uint64_t* core, int32_t* parent,
              int32_t* label, int32_t* status, hipStream_t stream);

// df.hip
int64_t jb_df_scratch_bytes(int64_t total, int64_t n);
int jb_df_weigh(const int64_t* row_ptr, int n, int64_t total, const int32_t* idx, float* val,
                const uint8_t* gw, int64_t* df, int64_t* diff, int64_t N0, int64_t L0, int update,
                void* scratch, int64_t scratch_bytes, int64_t* sel_len, hipStream_t st);

// fv_hash.hip
int jb_fv_hash(const uint8_t* buf, int64_t buf_len, int64_t buf_cap, const int64_t* datum_off,
               const int32_t* datum_len, const int64_t* row_ptr, int n, const void* srules,
               int n_srules, const void* nrules, int n_nrules, const uint8_t* blob, int blob_len,
               uint64_t H, int32_t* out_idx, float* out_val, int32_t* err, hipStream_t stream);

// fv_wide.hip
int jb_fvw_count(const uint8_t* buf, int64_t buf_len, const int64_t* datum_off,
                 const int32_t* datum_len, int n, const void* sr, int ns, const void* nr, int nn,
                 int ncomb, const uint8_t* blob, int64_t* base_cnt, int64_t* total_cnt,
                 int32_t* err, hipStream_t stream);
int jb_fvw_emit(const uint8_t* buf, int64_t buf_len, const int64_t* datum_off,
                const int32_t* datum_len, int n, const int64_t* row_ptr, const void* sr, int ns,
                const void* nr, int nn, int nbase, const uint8_t* blob, uint64_t H,
                int32_t* out_idx, float* out_val, uint64_t* out_h, void* out_name, uint8_t* out_gw,
                int32_t* err, hipStream_t stream);
int jb_fvw_comb(const uint8_t* buf, int n, const int64_t* row_ptr, const int64_t* base_cnt,
                const void* sr, const void* nr, const void* cr, int ncomb, const uint8_t* blob,
                uint64_t H, int32_t* idx, float* val, const uint64_t* hs, const void* names,
                hipStream_t stream);
int64_t jb_fvw_name_bytes();

// hot.hip
int jb_hot_detect(const int64_t* row_ptr, int n, const int32_t* fidx, int64_t max_slots,
                  int block_min, int min_count, int max_rows, int32_t* gkey, int32_t* gcnt,
                  int gcap, int32_t* hot_rows, int32_t* hot_n, hipStream_t stream);

// linear.hip
// hot_rows / hot_n (device): rows to keep in the block LDS replica (nullptr:
// none; only the concurrent modes with LC <= 64 use them); hot_rep: the
// delta shards (jb_hot_rep_bytes(), zero-initialised once, left zero). stats (device,
// 2 x u64, nullable): += samples that updated, samples with a valid label.
// touched (device, H bytes, nullable): set to 1 for every row an update wrote.
// mode kSerial (several streams, serial-equivalent result, serial.hip) needs
// n_max >= the batch's sample count and scratch of jb_serial_scratch_bytes_lc(n_max, LC).
int jb_linear_train(const int64_t* row_ptr, const int32_t* fidx, const float* fval,
                    const int32_t* labels, const int64_t* stream_ptr, int nstreams, float* W,
                    float* S, const int32_t* active, int LC, int method, float C, int mode,
                    const int32_t* hot_rows, const int32_t* hot_n, float* hot_rep,
                    int merge_every, int hot_waves, unsigned long long* stats, uint8_t* touched,
                    int64_t n_max, void* scratch, int64_t scratch_bytes, hipStream_t stream);
int jb_linear_train_bf16(const int64_t* row_ptr, const int32_t* fidx, const float* fval,
                         const int32_t* labels, const int64_t* stream_ptr, int nstreams,
                         uint16_t* W, float* S, const int32_t* active, int LC, int method, float C,
                         int mode, unsigned long long* stats, uint8_t* touched, void* scratch,
                         int64_t scratch_bytes, hipStream_t stream);
int64_t jb_hot_rep_bytes();
int jb_linear_classify(const int64_t* row_ptr, const int32_t* fidx, const float* fval,
                       int n_samples, const float* W, int LC, float* out, hipStream_t stream);
int jb_linear_classify_bf16(const int64_t* row_ptr, const int32_t* fidx, const float* fval,
                            int n_samples, const uint16_t* W, int LC, float* out,
                            hipStream_t stream);
int jb_scale(float* p, int64_t n, float a, hipStream_t stream);
int jb_mix_apply(float* w, const float* red, const float* loc, int64_t n, float inv_n,
                 hipStream_t stream);

// linear_chunked.hip
// The same train / classify with a run-time label capacity: LC any multiple
// of 256 from 256 to 16384 (anything else is refused before a launch).
// jb_linear_train / jb_linear_classify route label capacities above 1024
// here. W: float or (w_bf16 != 0) uint16 bf16 bit patterns. mode: kExact (one
// stream), kAtomic or kHogwild; waves per stream: 1, 4 or 16, 0 for the
// library's default (JUBATUS_LABEL_WAVES overrides the default).
int jb_linear_train_chunked(const int64_t* row_ptr, const int32_t* fidx, const float* fval,
                            const int32_t* labels, const int64_t* stream_ptr, int nstreams,
                            void* W, int w_bf16, float* P, const int32_t* active, int LC,
                            int method, float C, int mode, int waves, unsigned long long* stats,
                            uint8_t* touched, hipStream_t stream);
int jb_linear_classify_chunked(const int64_t* row_ptr, const int32_t* fidx, const float* fval,
                               int n_samples, const void* W, int w_bf16, int LC, float* out,
                               hipStream_t stream);

// lof.hip
int jb_lof_mark(int64_t nrows, int k, const int32_t* nb_slot, const int32_t* changed,
                const int32_t* nchanged, int clear_ok, uint8_t* ok, uint8_t* lrd_ok,
                hipStream_t stream);
int jb_lof_set_lists(int n, const int32_t* slots, const int32_t* cs, const float* cd, int kk, int k,
                     int ignore_same, int32_t* nb_slot, float* nb_dist, float* kdist, uint8_t* ok,
                     uint8_t* lrd_ok, int32_t* changed, int32_t* nchanged, hipStream_t stream);
int jb_lof_add_st(int p, const int32_t* cs, const float* cd, int nc, int k, int ignore_same,
                  int64_t nrows, int32_t* nb_slot, float* nb_dist, float* kdist, uint8_t* ok,
                  float* lrd, uint8_t* lrd_ok, int32_t* changed, int32_t* nchanged,
                  uint32_t* kstamp, uint32_t* lstamp, uint32_t epoch, uint32_t* out_host,
                  int max_missing, hipStream_t stream);
int jb_lof_add(int p, const int32_t* cs, const float* cd, int nc, int k, int ignore_same,
               int64_t nrows, int32_t* nb_slot, float* nb_dist, float* kdist, uint8_t* ok,
               float* lrd, uint8_t* lrd_ok, int32_t* changed, int32_t* nchanged,
               uint32_t* out_host, int max_missing, hipStream_t stream);
int jb_lof_add_many(int nadd, const int32_t* ps, const int32_t* cs, const float* cd,
                    const int32_t* nc, int stride, int k, int ignore_same, int32_t* nb_slot,
                    float* nb_dist, float* kdist, uint8_t* ok, float* lrd, uint8_t* lrd_ok,
                    int32_t* changed, int32_t* nchanged, uint32_t* kstamp, uint32_t* lstamp,
                    uint32_t epoch0, int32_t* cand, uint32_t* res, uint32_t* out_host,
                    int out_stride, int max_missing, unsigned long long* prof, hipStream_t stream,
                    int wait, uint32_t* chain);
int jb_lof_add_many_wait(int nadd, uint32_t* out_host, int out_stride, hipStream_t stream);
int jb_lof_score_st(const int32_t* ts, const float* td, int nt, int k, const int32_t* nb_slot,
                    const float* nb_dist, const float* kdist, const uint8_t* ok, float* lrd,
                    uint8_t* lrd_ok, int store_slot, const uint32_t* kstamp, uint32_t* lstamp,
                    uint32_t epoch, uint32_t* out_host, int max_missing, hipStream_t stream);
int jb_lof_score_many(int nq, const int32_t* ts, const float* td, const int32_t* nt, int stride,
                      int k, const int32_t* nb_slot, const float* nb_dist, const float* kdist,
                      const uint8_t* ok, float* lrd, uint8_t* lrd_ok, const uint32_t* kstamp,
                      uint32_t* lstamp, uint32_t epoch, uint32_t* out_host, int out_stride,
                      int max_missing, hipStream_t stream);
int jb_lof_score(const int32_t* ts, const float* td, int nt, int k, const int32_t* nb_slot,
                 const float* nb_dist, const float* kdist, const uint8_t* ok, float* lrd,
                 uint8_t* lrd_ok, int store_slot, uint32_t* out_host, int max_missing,
                 hipStream_t stream);
int jb_lof_invalidate(const int32_t* slots, int n, int64_t nrows, uint8_t* ok, uint8_t* lrd_ok,
                      hipStream_t stream);

// lsh.hip
int jb_signature(const int64_t* row_ptr, const int32_t* fidx, const float* fval, int n,
                 int hash_num, uint64_t seed, int mode, uint64_t* bits, float* norms,
                 hipStream_t stream);
int jb_hamming_scan(const uint64_t* qbits, const float* qnorm, int nq, const uint64_t* tbits,
                    const float* tnorm, const uint8_t* valid, int64_t nrows, int words,
                    int hash_num, int metric, float* out, hipStream_t stream);
int jb_sparse_scan(const int32_t* qidx, const float* qval, int qn, float qnorm2,
                   const int64_t* row_ptr, const int32_t* ridx, const float* rval,
                   const float* rnorm2, const uint8_t* valid, int64_t nrows, int metric,
                   float* out, hipStream_t stream);
int jb_lsh_query_direct(const int32_t* idx, const float* val, const int64_t* row_ptr, int nq,
                        int hash_num, uint64_t seed, int mode, int metric, const uint64_t* tbits,
                        const float* tnorm, const uint8_t* valid, int64_t nrows, int k,
                        uint64_t* qbits_scratch, float* qnorm_scratch, float* scratch_d,
                        int32_t* scratch_i, float* out_d_host, int32_t* out_i_host,
                        uint32_t* done_host, hipStream_t stream);
int jb_lsh_set_rows_direct(const int32_t* idx, const float* val, const int64_t* row_ptr, int n,
                           const int64_t* slots, int hash_num, uint64_t seed, int mode,
                           uint64_t* tbits, float* tnorm, uint8_t* valid, hipStream_t stream);
int jb_lsh_set_rows_staged(const int64_t* rp, const int64_t* slots, const int32_t* idx,
                           const float* val, int n, int hash_num, uint64_t seed, int mode,
                           uint64_t* tbits, float* tnorm, uint8_t* valid, hipStream_t stream);

// mix.hip
int jb_mix_take(uint8_t* touched, uint8_t* mark, int64_t H, hipStream_t st);
int64_t jb_mix_compact_temp_bytes(int64_t H);
int jb_mix_compact(const uint8_t* mark, int64_t H, int64_t* rows, int64_t* count, void* temp,
                   int64_t temp_bytes, hipStream_t st);
int jb_mix_gather(const float* W, const float* S, int LC, const int64_t* rows, int64_t n,
                  const int32_t* map, int Lc, float* snap, hipStream_t st);
int jb_mix_fold(float* W, float* S, int LC, const int64_t* rows, int64_t n, const int32_t* map,
                int Lc, const float* snap, const float* red, float inv_n, hipStream_t st);
int jb_mix_pair_sum(float* p, const float* q, int64_t n, hipStream_t st);
int jb_mix_pair_max(uint8_t* p, const uint8_t* q, int64_t n, hipStream_t st);
int jb_mix_pack_bf16(const float* snap, int64_t n, int Lc, int has_s, uint16_t* wb, float* sb,
                     hipStream_t st);
int jb_mix_unpack_bf16(const uint16_t* wb, const float* sb, int64_t n, int Lc, int has_s,
                       float* red, hipStream_t st);

// nn_reduce.hip
int jb_nn_reduce(const float* dist, const int32_t* row, int nq, int k, const float* targets,
                 int nrows, int mode, float alpha, float* out, int32_t* out_n,
                 hipStream_t stream);

// nn_vote.hip
// mode: 0 w = exp(-alpha d) (NN, euclidean), 1 w = 1 - d (cosine). row_lab:
// the label id of every slot, -1 for none. out: [nq, nlabels], all written.
int jb_nn_vote(const float* dist, const int32_t* row, int nq, int k, const int32_t* row_lab,
               int nrows, int nlabels, int mode, float alpha, float* out, hipStream_t stream);

// regression.hip
// method: models/linear_oracle.py METHOD_IDS (Method of jb_linear.hpp). PA
// launches regression_train_kernel, the other methods the templated
// regression_train_m_kernel. C is the regularization weight (perceptron: the
// learning rate). P: the precision table of CW / AROW / NHERD, null
// otherwise. slot_scratch: as many floats as fval, for those three methods;
// may be null when no sample has more than 256 slots.
int jb_regression_train_m(const int64_t* row_ptr, const int32_t* fidx, const float* fval,
                          const float* targets, const int64_t* stream_ptr, int nstreams, float* W,
                          float* P, float* stats, float* slot_scratch, int method, float C,
                          float eps, int concurrent, hipStream_t stream);
int jb_regression_estimate(const int64_t* row_ptr, const int32_t* fidx, const float* fval, int n,
                           const float* W, float* out, hipStream_t stream);

// regression_ordered.hip
// Samples 0 .. n_samples-1 applied in index order by one workgroup (the
// serial-equivalent training of a batch of requests laid out back to back),
// every method of jb_regression_train_m with its operands. win_slots: slot
// occurrences per LDS window, 0 for the default (4096); above the default:
// hipErrorInvalidValue. status: two int32, [0] 0 on success, else a code and
// [1] the index of the first sample that was not applied (codes in the
// kernel's header). A bad method, a missing P for CW / AROW / NHERD or a
// null status is hipErrorInvalidValue with nothing written; n_samples <= 0
// launches nothing and returns 0.
int jb_regression_train_ordered(const int64_t* row_ptr, const int32_t* fidx, const float* fval,
                                const float* targets, int64_t n_samples, float* W, float* P,
                                float* stats, float* slot_scratch, int method, float C, float eps,
                                int win_slots, int32_t* status, hipStream_t stream);

// scan.hip
int jb_scan_train(const uint8_t* buf, const int64_t* req_off, const int64_t* req_len,
                  const int64_t* sample_base, int R, const uint64_t* lt_hash,
                  const int32_t* lt_meta, int lt_cap, const uint8_t* lt_blob, int lt_blob_len,
                  int sps, int spn, int64_t* datum_off, int32_t* datum_len, int32_t* labels,
                  int64_t* row_ptr, int64_t* req_slots, uint32_t* hist, int nhist, int32_t* err,
                  uint8_t* empty_at, int64_t empty_off, int32_t* host_out, hipStream_t stream);
int jb_scan_train_profile(const uint8_t* buf, const int64_t* req_off, const int64_t* req_len,
                          const int64_t* sample_base, int R, const uint64_t* lt_hash,
                          const int32_t* lt_meta, int lt_cap, const uint8_t* lt_blob,
                          int lt_blob_len, int sps, int spn, int64_t* datum_off,
                          int32_t* datum_len, int32_t* labels, int64_t* row_ptr,
                          int64_t* req_slots, uint32_t* hist, int nhist, int32_t* err,
                          long long* prof, hipStream_t stream);

// serial.hip
int64_t jb_serial_scratch_bytes(int64_t n_max);
int64_t jb_serial_scratch_bytes_lc(int64_t n_max, int LC);
int jb_serial_scratch_forget(void* scratch);

// sparse_pool.hip
int jb_pool_scan(const int64_t* qptr, const int32_t* qidx, const float* qval, const double* qn2,
                 const int32_t* qslots, int nq, int qtot, const int64_t* r_off,
                 const int32_t* r_len, const double* r_n2, const uint8_t* valid, int64_t nrows,
                 const int32_t* p_idx, const float* p_val, int metric, int lpr, float* out,
                 hipStream_t stream);
int jb_pool_query_direct(const int32_t* idx, const float* val, const int64_t* row_ptr,
                         const int32_t* qslots, const int64_t* slot_len, int nq,
                         const int64_t* r_off, const int32_t* r_len, const double* r_n2,
                         const uint8_t* valid, int64_t nrows, const int32_t* p_idx,
                         const float* p_val, int metric, int lpr, int k, float* scores,
                         float* scratch_d, int32_t* scratch_i, float* out_d_host,
                         int32_t* out_i_host, uint32_t* done_host, hipStream_t stream);
int jb_pool_append(const uint8_t* pack, int n, int64_t nnz, int64_t base, int64_t* r_off,
                   int32_t* r_len, double* r_n2, uint8_t* valid, int32_t* p_idx, float* p_val,
                   hipStream_t stream);

// stepper.hip
int jb_stepper_error();
int jb_stepper_prof(unsigned long long* out);

// topk.hip
int jb_topk_blocks(int64_t nrows, int k);
int jb_topk(int mode, const uint64_t* qbits, const float* qnorm, int nq, const uint64_t* tbits,
            const float* tnorm, const uint8_t* valid, int64_t nrows, int words, int hash_num,
            int metric, const float* src_d, int flip, int k, float* scratch_d, int32_t* scratch_i,
            float* out_d, int32_t* out_i, hipStream_t stream);
int64_t jb_topk_direct_scratch(int nq);
int jb_topk_scratch_init(int32_t* scratch_i, hipStream_t stream);
int jb_topk_direct_query(const uint64_t* qbits, const float* qnorm, int nq, const uint64_t* tbits,
                         const float* tnorm, const uint8_t* valid, int64_t nrows, int words,
                         int hash_num, int metric, int k, float* scratch_d, int32_t* scratch_i,
                         float* out_d_host, int32_t* out_i_host, uint32_t* done_host,
                         hipStream_t stream);
int jb_topk_direct_query_path(const uint64_t* qbits, const float* qnorm, int nq,
                              const uint64_t* tbits, const float* tnorm, const uint8_t* valid,
                              int64_t nrows, int words, int hash_num, int metric, int k,
                              float* scratch_d, int32_t* scratch_i, float* out_d_host,
                              int32_t* out_i_host, uint32_t* done_host, int path,
                              hipStream_t stream);
void jb_topk_set_prof(long long* prof);
int jb_topk_scores_direct_path(const float* src_d, int flip, int nq, int64_t nrows, int k,
                               float* scratch_d, int32_t* scratch_i, float* out_d_host,
                               int32_t* out_i_host, uint32_t* done_host, int path_sel,
                               hipStream_t stream);
int jb_topk_scores_direct(const float* src_d, int flip, int nq, int64_t nrows, int k,
                          float* scratch_d, int32_t* scratch_i, float* out_d_host,
                          int32_t* out_i_host, uint32_t* done_host, hipStream_t stream);
int jb_topk_mq_stats(unsigned long long* out4);

// train_batch.hip
int64_t jb_train_batch_args_bytes();
// 0 ok, 1 a launch helper refused its arguments, 2 a HIP runtime error
int jb_train_batch_submit(const JbTrainBatch* a);
int64_t jb_event_create();
int jb_event_destroy(int64_t e);
int jb_event_record(int64_t e, hipStream_t stream);
int jb_stream_wait_event(hipStream_t stream, int64_t e);
int jb_event_query(int64_t e);
int jb_event_sync(int64_t e);

// vcommit.hip
int64_t jb_vcommit_fixed_bytes();

// Internal: called from one .hip file into another, by neither ctypes nor a
// server.
// stepper.hip: one stream of samples applied in order from an LDS row cache
int jb_stepper_enabled();
int jb_stepper_train(const int64_t* row_ptr, const int32_t* fidx, const float* fval,
                     const int32_t* labels, const int64_t* range, float* W, float* P,
                     const int32_t* active, int LC, int method, float C,
                     unsigned long long* stats, uint8_t* touched, int* err, hipStream_t stream);
int jb_stepper_chunk(const int64_t* row_ptr, const int32_t* fidx, const float* fval,
                     const int32_t* labels, float* W, float* P, const int32_t* active, int LC,
                     int method, float C, unsigned long long* stats, uint8_t* touched,
                     int64_t* vst, int64_t* vtail, hipStream_t stream);
int jb_stepper_cand(const int64_t* row_ptr, const int32_t* fidx, const float* fval,
                    const int32_t* labels, float* W, float* P, const int32_t* active, int LC,
                    int method, float C, int64_t* vst, const int4* aux, int32_t* g_key,
                    float* g_rmax, float* g_dw, float* g_dp, hipStream_t stream);
// vcommit.hip: the verified committer (label capacities <= 64)
int jb_vcommit_prepare(const int64_t* row_ptr, const int32_t* fidx, const float* fval,
                       const int32_t* labels, const int64_t* stream_ptr, int nstreams,
                       int64_t n_max, float* W, float* S, const int32_t* active, int LC,
                       int method, float C, unsigned long long* stats, uint8_t* touched,
                       void* scratch, int nseg, hipStream_t stream);
// serial.hip
int jb_serial_prepare(const int64_t* row_ptr, const int32_t* fidx, const float* fval,
                      const int32_t* labels, const int64_t* stream_ptr, int nstreams,
                      int64_t n_max, float* W, float* S, const int32_t* active, int LC, int method,
                      float C, unsigned long long* stats, uint8_t* touched, void* scratch,
                      int64_t scratch_bytes, int bail_after, hipStream_t stream);

}

#endif  // JUBATUS_AMD_CSRC_HIP_JB_HIP_API_H_
