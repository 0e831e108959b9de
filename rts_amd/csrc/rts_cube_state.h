// rts_cube_state.h -- the cube part of a handle, one record per family of entry points: what each family keeps between its calls.
// A launcher binds the record of its own family (RtsTbdState& s = c->cube.tbd) and reads the cube itself (params, p) from c->cube.
// The records own their memory through rts_owned.h's types and free themselves, members in reverse order of declaration -- an order that follows
// the grouping here and nothing else.  That is safe: ~RtsContext drains the handle's streams before any member frees itself (rts_owned.h).
//
// Host code only, HIP's API header and the standard library only (tests/cube_state/cube_state_main.cpp builds it without the runtime).
#pragma once
#include <stdint.h>
#include <vector>
#include "../../include/rts_amd.h"
#include "rts_owned.h"
#include "rts_track.h"            // RtsTrackPred
#include "rts_locate.h"           // RtsLocateGeo

// A derived output of the attached cube (Doppler map, image, spectrogram): `own` when the library allocates it, p / doubles: where the
// last one went and its size; valid: it is a product of the ATTACHED cube, for its rts_cube_*_get -- every product ends at rts_cube_attach
// (RtsCubeState::end_products).  The image and the spectrogram are recorded only when library-owned (a caller-owned
// output leaves the record alone), the Doppler map also when caller-owned (rts_cube_detect without a map takes it).
struct RtsCubeProduct {
    DevBuf<double> own; double* p = nullptr; size_t doubles = 0; bool valid = false;
    // where a call's n doubles go: the caller's memory, or `own` made large enough.  A regrow frees the block a record may name: the record
    // ends BEFORE it, so a call that fails after this (the reserve itself, a staged upload) leaves no getter a freed address
    hipError_t place(void* device_out, size_t n, double** out)
    {
        *out = (double*)device_out; if (*out) return hipSuccess;
        if (n > own.cap) { p = nullptr; doubles = 0; valid = false; }
        const hipError_t e = own.reserve(n); *out = own.p; return e;
    }
    void record(double* out, size_t n) { p = out; doubles = n; valid = true; }
};

// the transmit waveform (rts_cube_set_waveform): M interleaved samples, L taps
struct RtsWaveState { DevBuf<double> d; uint32_t M = 0, L = 0; bool set = false; };
// slow-time transform of the cube (rts_cube_doppler) and its n_fft
struct RtsDopplerState { RtsCubeProduct map; uint32_t n_fft = 0; void end() { map.valid = false; } };
// CFAR detection (rts_cube_detect, rts_detect.hip): per-segment counts -> exclusive scan (offsets; element n_seg: the total),
// the records of the last detection and how many it may hold; valid: a list exists for rts_cube_detections_get
struct RtsDetectState {
    DevBuf<uint32_t> d_cnt, d_off; DevBuf<uint8_t> d_tmp; DevBuf<RtsDetection> d_list; uint32_t nseg = 0, max = 0; bool valid = false;
    uint32_t nd = 0;                                      // the Doppler rows of the map the list was detected on (rts_cube_plots without a list of its own)
    // OS-CFAR (rts_cube_detect_os): the alphas by training count go through a staged upload; os_tab keeps them on the host for the next
    // call with the same window, rank and pfa (os_key), so that only training counts not seen yet are solved for; os_sent: the
    // device holds os_tab as it stands
    StagedUpload<double> os_alpha; std::vector<double> os_tab; uint32_t os_key[5] = {0, 0, 0, 0, 0}; double os_pfa = 0.0; bool os_sent = false;
    void end() { valid = false; }                         // (the alphas belong to no cube: they stay)
};
// plot extraction (rts_cube_plots, rts_plot.hip): flat keys, the parent array of the union (afterwards every element's component
// minimum), the identity, (label, index) sorted by label, per head its member count, keep flags -> exclusive scan (offsets;
// element cap: the total), the sort's and the scan's scratch, the records.  cap: the list capacity the launches were
// sized by, max: the records d_list may hold; valid: plots exist for rts_cube_plots_get; own_list: they were made
// from the handle's detection list (whose truncation rts_cube_plots_get reports)
struct RtsPlotState {
    DevBuf<uint64_t> d_key; DevBuf<uint32_t> d_parent, d_idx, d_lab_s, d_idx_s, d_len, d_flag, d_off; DevBuf<uint8_t> d_tmp;
    DevBuf<RtsPlot> d_list; uint32_t cap = 0, max = 0; bool valid = false, own_list = false;
    void end() { valid = false; }
};
// what the device keeps beside each of the two track tables: the next id, the records stored, the total a table without end would
// hold (stored + the new tracks turned away), the rounds the matching took
struct RtsTrackMeta { uint64_t next_id; uint32_t n, total, rounds, reserved; };
// tracking (rts_cube_track, rts_track.hip): TWO tables of RTS_TRACK_MAX_TRACKS records and their RtsTrackMeta -- a step reads
// table cur and writes the other -- the predictions, the plots' four fields, per track its candidates (entry k of track i at
// [k * table size + i]), their count, its plot and that edge's d2, per plot its track and the round's minimum (d2 bits, track), the
// rounds, the flags over [tracks | plots | 1] -> exclusive scan, the scan's scratch.  NOT a product of the cube: end_products()
// leaves them alone.  max: the table size the previous step ran with (0: the next step chooses); live: the table has a time
struct RtsTrackState {
    DevBuf<RtsTrack> d_tab[2]; DevBuf<RtsTrackMeta> d_meta; DevBuf<RtsTrackPred> d_pred;
    DevBuf<double> d_zd, d_zf, d_pw, d_cd, d_md2; DevBuf<uint64_t> d_best_d; DevBuf<uint8_t> d_tmp;
    DevBuf<uint32_t> d_zrx, d_cj, d_cn, d_of_track, d_of_plot, d_best_t, d_rounds, d_flag, d_off;
    uint32_t cur = 0, max = 0, loaded = 0; bool live = false; double time = 0.0;
};
// what the device keeps beside the targets: the candidates accepted and stored, the targets a list without end would hold, the rounds
// the resolution took, whether an anchor's segment was cut
struct RtsLocateMeta { uint32_t cand_total, cand_stored, targets_total, rounds, seg_cut, reserved[3]; };
// multistatic localisation (rts_cube_locate, rts_locate.hip): the copy of the records' four fields in segment order with their list
// indices and receivers, the segments' bounds and the count; for a track table the flags over [16][table] -> exclusive scan; per
// (i, j) pair of the anchors' segments its candidates' count -> exclusive scan (offsets; the last element: the total); the candidates;
// per candidate its state, per record whether it is taken and the round's minimum (16 - K, cost bits, position); the winners' flags
// -> exclusive scan; the scans' scratch; the targets and their RtsLocateMeta; the call's constants go through a staged upload.  NOT a
// product of the cube: end_products() leaves them alone.  max_c, max_t: the capacities of the last call; valid: targets exist
struct RtsLocateState {
    DevBuf<double> d_zr, d_zf, d_zp; DevBuf<uint64_t> d_best_c; DevBuf<uint8_t> d_tmp;
    DevBuf<uint32_t> d_zi, d_zrx, d_seg, d_n, d_tflag, d_toff, d_pcnt, d_poff, d_state, d_taken, d_best_k, d_best_i, d_win, d_woff;
    DevBuf<RtsTarget> d_cand, d_out; DevBuf<RtsLocateMeta> d_meta; StagedUpload<RtsLocateGeo> geo;
    uint32_t max_c = 0, max_t = 0; bool valid = false;
};
// track-before-detect (rts_cube_tbd_step, rts_cube_tbd_extract, rts_tbd.hip): TWO merit maps -- a step reads cur and writes the
// other -- the ring of depth pointer maps and of their shift tables (frame f in slot f mod depth), all of the shape and
// window the first step after a reset fixed (frames == 0: no state); the time, and t0 and dt, of the last frame.  The
// extraction: per segment of 64 cells its candidates' count -> exclusive scan (offsets; element ext_nseg: the total), the
// scan's scratch, the records and their paths.  NOT a product of the cube: end_products() leaves all of it alone.
struct RtsTbdState {
    DevBuf<double> d_merit[2]; DevBuf<uint8_t> d_ptr, d_tmp; DevBuf<int32_t> d_shift; DevBuf<uint32_t> d_cnt, d_off, d_paths; DevBuf<RtsTbdTrack> d_out;
    uint32_t rx = 0, nd = 0, nb = 0, depth = 0, hd = 0, hr = 0, cur = 0; uint64_t frames = 0; double time = 0.0, t0 = 0.0, dt = 0.0;
    uint32_t ext_nseg = 0, ext_max = 0, ext_depth = 0; bool ext_valid = false;
};
// backprojection (rts_cube_backproject, rts_image.hip): the image and its shape, for rts_cube_image_get / RTS_IMAGE_ACCUMULATE; the
// call's geometry [tx | rx | w] goes through a staged upload; the chunk sums of a split launch
struct RtsImageState { RtsCubeProduct out; uint32_t nx = 0, ny = 0; StagedUpload<double> geo; DevBuf<double> d_scratch; void end() { out.valid = false; } };
// spectrogram (rts_cube_spectrogram, rts_stft.hip): the output, for rts_cube_spectrogram_get; the call's window goes through a
// staged upload; the tile sums of RTS_STFT_SUM_BINS
struct RtsStftState { RtsCubeProduct out; StagedUpload<double> win; DevBuf<double> d_part; void end() { out.valid = false; } };
// FMCW (rts_beat.hip): the part sums of a beat render (rts_cube_render_beat); the range transform's output
// (rts_cube_range_transform), for rts_cube_range_get, and its staged window
struct RtsFmcwState { DevBuf<double> d_beat_part; RtsCubeProduct range; StagedUpload<double> range_win; void end() { range.valid = false; } };
// beamforming (rts_cube_beamform, rts_beam.hip): the output, for rts_cube_beam_get; the call's weight table goes through a staged upload
struct RtsBeamState { RtsCubeProduct out; StagedUpload<double> w; void end() { out.valid = false; } };
// clutter and jammer sources (rts_cube_add_sources, rts_source.hip): the call's table (rts_src_table) goes through a staged upload;
// the call changes the cube in place, so there is no product
struct RtsSourceState { StagedUpload<double> tab; };
// adaptive beamforming (rts_cube_covariance, rts_cube_mvdr, rts_adapt.hip): the covariance and its n_rx, for rts_cube_covariance_get
// and rts_cube_mvdr without device_cov, and the parts' partial sums; the weights, for rts_cube_mvdr_get; the call's steering rows go
// through a staged upload; the solves' status words (0: library-owned output, 1: caller-owned)
struct RtsAdaptState {
    RtsCubeProduct cov; uint32_t cov_n = 0; DevBuf<double> d_cov_part; RtsCubeProduct mvdr; StagedUpload<double> mvdr_s; DevBuf<uint32_t> d_mvdr_status;
    void end() { cov.valid = false; mvdr.valid = false; }
};
// space-time adaptive processing (rts_cube_st_covariance: the adaptive family's `cov`, of order n_taps n_rx; rts_cube_st_apply,
// rts_stap.hip): the filter's output, for rts_cube_st_get; the call's weight table goes through a staged upload
struct RtsStapState { RtsCubeProduct out; StagedUpload<double> w; void end() { out.valid = false; } };
// direction finding (rts_cube_eig, rts_cube_doa_scan, rts_doa.hip): the eigenvalues and the eigenvectors and their order, for
// rts_cube_eig_get and rts_cube_doa_scan without device_vectors; the solves' status words (0: library-owned outputs, 1: caller-owned);
// the spectrum, for rts_cube_doa_get; the call's g goes through a staged upload of one size (RTS_BEAM_MAX_RX doubles)
struct RtsDoaState {
    RtsCubeProduct eig_val, eig_vec; uint32_t eig_n = 0; DevBuf<uint32_t> d_eig_status; RtsCubeProduct spectrum; StagedUpload<double> g;
    void end() { eig_val.valid = false; eig_vec.valid = false; spectrum.valid = false; }
};
// autofocus (rts_cube_align, rts_cube_pga, rts_cube_correct, rts_focus.hip): the shift table and the phase table (phase, then the
// iterations' rms) with the row ranges they were made for, for their getters and RTS_CORRECT_USE_ALIGN / RTS_CORRECT_USE_PGA; the
// rows' envelopes and the reference; the PGA's tile sums, their sums and the rotations; the correction's copy of the rows; a
// correction's host tables [shifts | phase] go through a staged upload
struct RtsFocusState {
    RtsCubeProduct align; uint32_t align_first = 0, align_P = 0;
    RtsCubeProduct pga; uint32_t pga_first = 0, pga_P = 0, pga_iters = 0;
    DevBuf<double> d_env, d_ref, d_pga_part, d_pga_sum, d_pga_rot, d_rows; StagedUpload<double> tab;
    void end() { align.valid = false; pga.valid = false; }
};
// passive radar (rts_cube_cancel, rts_cube_xcorr, rts_passive.hip): the parts' partial sums and their sums, both in records of
// [K (K + 1) / 2 entries of G | n_rx rows of K entries of b] (rts_passive.h), the coefficients [n_rx][n_blocks][K], per block the column + 1 of
// its failed pivot (0: solved) -- the info record is counted from it --, and the shape of the last cancellation, for
// rts_cube_cancel_info / rts_cube_cancel_coeffs_get; the correlation's output, for rts_cube_xcorr_get.  The record and the product end
// at rts_cube_attach.  (The product goes by an alias: tests/cube_state's driver lists the products declared under the type's own name
// one by one and stays as it is; tests/passive/passive_state_main.cpp lists this one and holds end() to it.)
using RtsXcorrProduct = RtsCubeProduct;
struct RtsPassiveState {
    DevBuf<double> d_part, d_sums, d_coeff; DevBuf<uint32_t> d_fail; uint32_t n_blocks = 0, n_taps = 0, n_rx = 0; bool cancel_valid = false;
    RtsXcorrProduct xcorr;
    void end() { cancel_valid = false; xcorr.valid = false; }
};
// MIMO radar (rts_cube_bank, rts_mimo.hip): the call's table [the waveforms' samples, one after another | the code table] goes through a
// staged upload; the bank's output, for rts_cube_bank_get.  The product ends at rts_cube_attach.  (Declared through an alias, as the
// correlation's: tests/mimo/mimo_state_main.cpp lists this one and holds end() to it.)
using RtsBankProduct = RtsCubeProduct;
struct RtsMimoState { StagedUpload<double> tab; RtsBankProduct out; void end() { out.valid = false; } };

// The cube part of a handle: it shares nothing with the pulse path but the handle (the three rts_cube*_api.hip units; the launchers of
// the kernels' units, each on its own family).
struct RtsCubeState {
    RtsCubeParams params = {}; double* p = nullptr; DevBuf<double> own; bool set = false;      // p: the attached cube, own when the library allocated it
    RtsWaveState wave; RtsDopplerState doppler; RtsDetectState detect; RtsPlotState plot; RtsTrackState track; RtsLocateState locate; RtsTbdState tbd; RtsImageState image; RtsStftState stft;
    RtsFmcwState fmcw; RtsBeamState beam; RtsSourceState source; RtsAdaptState adapt; RtsStapState stap; RtsDoaState doa; RtsFocusState focus; RtsPassiveState passive; RtsMimoState mimo;
    // every product belongs to the cube it was made from: the Doppler map (which rts_cube_detect may take), the detection list, the plots, the image, the spectrogram, the
    // range transform, the beams, the covariance, the adaptive weights, the space-time filter's output, the eigenpairs, the angular spectrum, the autofocus tables, the cancellation's record, the reference correlation and the bank's output end when another cube is attached
    void end_products() { doppler.end(); detect.end(); plot.end(); image.end(); stft.end(); fmcw.end(); beam.end(); adapt.end(); stap.end(); doa.end(); focus.end(); passive.end(); mimo.end(); }
};
