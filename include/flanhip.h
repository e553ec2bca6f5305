/* flanhip.h -- C ABI of the MI355X (gfx950) phase-vocoder hot path.
 *
 * This is the drop-in boundary: plain pointers and sizes, no C++ or torch types.  The reference (loganmcbroom/Flan)
 * has no FFI layer -- the path is a set of C++ member functions -- so each entry point below names the reference
 * member function it stands in for (paths relative to /root/reference/src/flan).  The C++ host classes in
 * include/flan/ (flan::Audio, flan::PV, flan::Function) are written on top of exactly these calls; INTEGRATION.md
 * shows the binding a Flan maintainer would add.
 *
 * Conventions
 *   - every function returns FLANHIP_OK (0) or a negative FLANHIP_ERR_*; nothing throws; flanhip_last_error() gives
 *     the text of the last failure on the calling thread.
 *   - host entry points (no suffix) take HOST pointers, do H2D / kernels / D2H on the current device and return
 *     when the result is in the caller's buffer.  The caller owns all host memory.
 *   - device entry points (_dev) take DEVICE pointers plus a hipStream_t passed as void* (NULL = default stream),
 *     enqueue work and return without synchronising; results chain on-device so a
 *     convert_to_PV -> stretch -> convert_to_audio pipeline never leaves HBM.
 *   - layouts are the reference's: audio float[channel][frame] (Audio/AudioBuffer.cpp:479-482),
 *     PV flanhip_MF[channel][frame][bin] (PV/PVBuffer.cpp:526-529).  All indices are 64-bit here (the reference's
 *     int32 product overflows above 2^31 MFs, PV/PVBuffer.cpp:19-22).
 *   - `cancel` (may be NULL) is the reference's canceller (defines.h:49-62): polled between kernel batches; when it
 *     reads non-zero the call stops and returns FLANHIP_ERR_CANCELLED (the C++ layer then returns a null object).
 *   - there is NO CPU fallback: without a usable HIP device every compute entry point fails with
 *     FLANHIP_ERR_NO_DEVICE.
 */
#ifndef FLANHIP_H
#define FLANHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FLANHIP_OK                 0
#define FLANHIP_ERR_INVALID_ARG   -1   /* null pointer, non-positive size, window > dft ...                    */
#define FLANHIP_ERR_UNSUPPORTED   -2   /* dft size odd, below 4 or above 2^20, chain constraints ...           */
#define FLANHIP_ERR_HIP           -3   /* a HIP runtime call failed; see flanhip_last_error()                  */
#define FLANHIP_ERR_CANCELLED     -4   /* the canceller was raised                                              */
#define FLANHIP_ERR_NO_DEVICE     -5   /* no gfx950 device visible                                              */

/* defines.h:31-35  struct MF { Magnitude m; Frequency f; } */
typedef struct flanhip_MF { float m; float f; } flanhip_MF;

/* ---- library / device ------------------------------------------------------------------------------------ */
int          flanhip_version(void);                 /* 10000*major + 100*minor + patch */
const char * flanhip_last_error(void);
int          flanhip_device_count(void);            /* 0 when no device; never fails   */
int          flanhip_set_device(int device);
int          flanhip_get_device(int * device);      /* the calling thread's current device */

/* ---- shape helpers (pure host arithmetic, usable without a device) ---------------------------------------- */
/* Conversions/AudioPV.cpp:17   numHops = ceil( num_frames / hop ) + 1, INTEGER division */
int64_t flanhip_num_pv_frames(int64_t num_audio_frames, int hop);
/* PV/PVBuffer.cpp:381-384      get_hop_size() = Frame( sample_rate / analysis_rate )     */
int     flanhip_hop_size(float sample_rate, float analysis_rate);
/* PV/PVModify.cpp:312-316      ceil( time_to_frame( max of the time map ) ), from a host grid float[F][bins] */
int64_t flanhip_modify_time_out_frames(const float * mod_seconds, int64_t num_frames, int num_bins, float sample_rate, int hop);

/* ---- device memory plumbing (so that C / C++ / ctypes callers need no HIP headers) ------------------------ */
int flanhip_malloc(void ** dptr, size_t bytes);
int flanhip_free(void * dptr);
int flanhip_memcpy_h2d(void * dst, const void * src, size_t bytes, void * stream);
int flanhip_memcpy_d2h(void * dst, const void * src, size_t bytes, void * stream);
int flanhip_memset(void * dst, int value, size_t bytes, void * stream);
int flanhip_stream_synchronize(void * stream);
/* Cancellation INSIDE a launch (defines.h:49-62: the reference polls its flag once per frame, AudioPV.cpp:49,115).  Wait for `stream` like
 * flanhip_stream_synchronize, but poll the caller's flag meanwhile; when it rises, the conversion kernels this thread has launched stop
 * starting chains -- a block of the FFT kernels walks at most 512 frames (~3 ms), the direct-sum kernels look every few batches of frames --
 * and the call returns FLANHIP_ERR_CANCELLED once the stream has drained (outputs are then unspecified).  Returns FLANHIP_OK when the work
 * completed without the flag rising.  The _fn form takes a predicate (non-zero = cancel) instead of an int flag, for callers whose flag is
 * not an int (the C++ classes' std::atomic<bool>&).  The host-buffer entry points (flanhip_analyze, flanhip_synthesize) wait this way with
 * their own `cancel` argument. */
/* Scope: the wait on `stream` stops the conversion kernels THIS thread has launched on THAT stream; what the thread has in flight on its
 * other streams (and what other threads have in flight anywhere) runs to completion.  (A thread that uses more than 64 streams at once on
 * one device shares cancel words between them: such a stream may be stopped together with another one of the same thread.) */
int flanhip_wait_cancellable(void * stream, volatile int * cancel);
int flanhip_wait_cancellable_fn(void * stream, int (*poll)(void * user), void * user);
/* Transfers between ordinary (pageable) host memory and the device, synchronous: what the host entry points below
 * (flanhip_analyze, flanhip_synthesize, ...) use for the caller's buffers.  A download first lets a pool of worker threads fault
 * the destination's pages in together (a fresh allocation costs more to fault in on one thread than to fill over the link), then
 * both directions are the runtime's copies, which run at the link's rate.  flanhip_touch_pages is that first step on its own
 * (it writes a zero into every page: for memory about to be overwritten).  flanhip_parallel_for runs fn( ctx, i ), i in [0, n), on
 * those workers and the calling thread (as many threads as the process may use; FLAN_HOST_THREADS overrides); a region started
 * while another runs, or from inside one, runs inline.  fn must not throw. */
int flanhip_upload(void * d_dst, const void * src, size_t bytes);
int flanhip_download(void * dst, const void * d_src, size_t bytes);
int flanhip_touch_pages(void * ptr, size_t bytes);
int flanhip_host_workers(void);
int flanhip_parallel_for(int n_tasks, void (*fn)(void *, int), void * ctx);
/* a stream of the caller's own (e.g. one per copy direction, so that a download and an upload overlap); every entry point
 * that takes `void * stream` accepts it, NULL stays the default stream */
int flanhip_stream_create(void ** stream);
int flanhip_stream_destroy(void * stream);
/* page-locked host memory: what a caller samples a Function grid into (Function.h:155-171) so that the upload runs at the
 * link's rate instead of through the runtime's staging copy.  Needs a device. */
int flanhip_host_malloc(void ** hptr, size_t bytes);
int flanhip_host_free(void * hptr);

/* ---- Audio::convert_to_PV  (Conversions/AudioPV.cpp:12-78, phase_vocoder.cpp:5-53, WindowFunctions.cpp:10-13) - */
/* audio: float[ch][n]; out: MF[ch][F][dft/2+1] with F = flanhip_num_pv_frames(n, hop), written to *num_pv_frames. */
/* dft_size: any even size in [4, 2^20] with window_size <= dft_size (FFTHelper.cpp:16-26 hands the caller's size to FFTW as it is).  Which
 * kernels serve a size: powers of two in [32, 16384] tuned or LDS-resident FFT kernels; other sizes whose half factors
 * into 2 ... 13, up to 16384, mixed-radix FFT kernels; sizes above 16384 whose half is C1 <= 256 times a product of 2 ... 13 up to 4096 (32768 ... 2^20,
 * 20000, 44100, 48000 ...) residue-pair kernels; every other size whose half is 64 ... 131072 (a larger prime factor) Bluestein's chirp-z form -- in LDS up
 * to dft 8192, in device memory above (convert_to_PV takes that stretch from the stream: hipMallocAsync / hipFreeAsync around the launch); anything else
 * the transform's definition summed in fp64 (pv_kernels_any.h): O( window x bins ) per frame, same results.  flanhip_synthesize_workspace_bytes includes
 * the scratch a size needs (direct sums: one PV's worth of spectra + frames x window floats; residue pairs: C1 / 2 + 1 output streams; chirp-z in
 * device memory: two frames of the transform's length per chain). */
int flanhip_analyze(const float * audio, int64_t num_channels, int64_t num_audio_frames, float sample_rate,
                    int window_size, int hop, int dft_size,
                    flanhip_MF * out, int64_t * num_pv_frames, volatile int * cancel);
int flanhip_analyze_dev(const float * d_audio, int64_t num_channels, int64_t num_audio_frames, float sample_rate,
                        int window_size, int hop, int dft_size,
                        flanhip_MF * d_out, void * stream);

/* ---- PV::convert_to_audio  (Conversions/AudioPV.cpp:86-139, phase_vocoder.cpp:55-61) ------------------------- */
/* pv: MF[ch][F][bins]; out: float[ch][F*hop], hop = flanhip_hop_size(sr, analysis_rate).
 * *nan_flag (may be NULL) is set to 1 when the buffer holds a NaN/Inf (PV/PVBuffer.cpp:44-50; the reference prints
 * a warning and carries on, AudioPV.cpp:88-89 -- so do we). */
int flanhip_synthesize(const flanhip_MF * pv, int64_t num_channels, int64_t num_pv_frames, int num_bins,
                       float sample_rate, float analysis_rate, int window_size,
                       float * out, int * nan_flag, volatile int * cancel);
/* Device form.  d_workspace must hold flanhip_synthesize_workspace_bytes(...) bytes for the SAME arguments (and the same
 * setting of the debug knobs FLANHIP_CHAIN_LEN / FLANHIP_TARGET_CHAINS / FLANHIP_FORCE_GENERIC, which change the layout and
 * are read per call); d_nan_flag (may be NULL) is a device int that is OR-ed with 1 on NaN/Inf (the caller zeroes it), and with 2 by
 * flanhip_synthesize_dev_fused when the workspace does not hold what the library noted its last producer left there (two callers racing on one
 * workspace between an analysis and its synthesis: the output is then not to be trusted). */
size_t flanhip_synthesize_workspace_bytes(int64_t num_channels, int64_t num_pv_frames, int num_bins,
                                          float sample_rate, float analysis_rate, int window_size);
int flanhip_synthesize_dev(const flanhip_MF * d_pv, int64_t num_channels, int64_t num_pv_frames, int num_bins,
                           float sample_rate, float analysis_rate, int window_size,
                           float * d_out, void * d_workspace, int * d_nan_flag, void * stream);

/* Fused round trip (convert_to_PV immediately followed, possibly after read-only use, by convert_to_audio of the SAME,
 * unmodified PV): the analysis kernel also leaves in `d_synth_workspace` (sized by flanhip_synthesize_workspace_bytes for the
 * PV it produces) what synthesis' pre-pass would compute -- the per-chain sums of the phase increments and the NaN/Inf flag --
 * and flanhip_synthesize_dev_fused starts from them instead of re-reading the PV.  Results are identical to the unfused pair. */
int flanhip_analyze_dev_fused(const float * d_audio, int64_t num_channels, int64_t num_audio_frames, float sample_rate,
                              int window_size, int hop, int dft_size,
                              flanhip_MF * d_out, void * d_synth_workspace, void * stream);
int flanhip_synthesize_dev_fused(const flanhip_MF * d_pv, int64_t num_channels, int64_t num_pv_frames, int num_bins,
                                 float sample_rate, float analysis_rate, int window_size,
                                 float * d_out, void * d_workspace, int * d_nan_flag, void * stream);
/* ... and for a PV whose workspace MAY hold the pre-pass (flanhip_modify_time_dev_fused): the pre-pass kernel is launched and
 * retires at once when the sums are there.  The hand-over is consumed: a second call on the same workspace runs the pre-pass. */
int flanhip_synthesize_dev_fused_checked(const flanhip_MF * d_pv, int64_t num_channels, int64_t num_pv_frames, int num_bins,
                                         float sample_rate, float analysis_rate, int window_size,
                                         float * d_out, void * d_workspace, int * d_nan_flag, void * stream);

/* The same call with the kernels it launches as a per-call argument: presummed 0 = flanhip_synthesize_dev, 1 = _fused, 2 = _fused_checked;
 * stages: bit 0 k_phase_sums, 1 k_phase_scan, 2 k_synthesize, 3 k_ola_fixup (0xF: all of them, i.e. the plain entry points above).
 * For timing ONE kernel of a call with events (bench.py's roofline object); the output is only meaningful with all four. */
int flanhip_synthesize_dev_stages(const flanhip_MF * d_pv, int64_t num_channels, int64_t num_pv_frames, int num_bins,
                                  float sample_rate, float analysis_rate, int window_size,
                                  float * d_out, void * d_workspace, int * d_nan_flag, int presummed, int stages, void * stream);

/* Test / A-B hooks, PER CALLING THREAD (thread-local, all 0 = off by default; the library's own paths and the C++ classes never set them, and
 * no entry point reads an environment variable).  A thread that sets one changes how ITS later calls are cut or routed -- never the results
 * beyond the documented tolerances (tests/test_gpu_conversions.py holds that) -- and must size a workspace under the same settings it
 * converts with (chain length and chain count decide the layout). */
#define FLANHIP_DEBUG_CHAIN_LEN       0   /* frames per chain */
#define FLANHIP_DEBUG_TARGET_CHAINS   1   /* chains the tuned kernels are cut for (default: what the device holds at once) */
#define FLANHIP_DEBUG_FORCE_GENERIC   2   /* 1: never the tuned dft 2048 / 4096 kernels */
#define FLANHIP_DEBUG_NO_FAST_DIV     3   /* 1: hardware division by the analysis rate */
#define FLANHIP_DEBUG_ANA_VARIANT     4   /* dft 2048 analysis: ablated instantiations (diagnostic builds only) */
#define FLANHIP_DEBUG_SYN_VARIANT     5   /* dft 2048 synthesis: 2 = behind the scan kernel even where it could work out its own carries; ablations */
#define FLANHIP_DEBUG_ANA4096_OLD     6   /* 1: the generic block-per-chain analysis kernel (pv_kernels.h) instead of the dft 4096 team kernel (A/B predecessor) */
#define FLANHIP_DEBUG_SYN4096_OLD     7   /* 1: the generic dft 4096 synthesis kernel */
#define FLANHIP_DEBUG_RESAMPLE_DIRECT 8   /* 1: Audio::resample's 2:1 block convolver always as direct fp64 sums in the checker's operation order
                                           * (default: fp64 overlap-save FFT convolution, the reference's own method, r8brain/CDSPBlockConvolver.h:242-344,
                                           * for float streams of at least 8 blocks); 2: the convolver's 256-thread radix-16 generation (A/B predecessor) */
#define FLANHIP_DEBUG_FORCE_DIRECT    9   /* 1: dft sizes without power-of-two kernels as direct fp64 sums (the transform's definition: pv_kernels_any.h),
                                           * never the mixed-radix FFT kernels (pv_kernels_mr.h): the checker-order path, for A/B */
#define FLANHIP_DEBUG_INLINE_FIXUP   10   /* the dft 512 ... 16384 synthesis kernels adding the overlaps of neighbouring chains themselves (a tagged word per boundary, the
                                           * head's owner publishing from inside its frame loop; agent-scope side buffers) instead of k_ola_fixup in a launch of
                                           * its own -- the same sums.  0: where the chains are long enough (the default), 1: always, 2: never */
#define FLANHIP_DEBUG_WIDE_OFFSETS   11   /* 1: kernels that choose 32-bit element offsets for grids below 2^30 elements (k_stretch_map) take their 64-bit
                                           * form whatever the size: the path of multi-gigabyte grids, testable on small ones */
#define FLANHIP_DEBUG_NO_SUB         12   /* 1: dft 512 / 256 / 128 never on the kernels with several chains per wavefront (pv_kernels_sub.h, round 6): A/B against
                                             the one-wavefront kernels (dft 512) / the generic ones (dft 256) */
void flanhip_debug_option(int which, int value);
/* Scratch (private memory) bytes per lane of a kernel whose hand-counted s_waitcnt values are only right while the compiler emits no memory
 * operation of its own on that path -- a spill or reload is one (tests/test_gpu_processors.py holds them to 0).  which: 0 / 1 = k_stretch_map with
 * 32-bit / 64-bit row offsets.  Negative: error. */
int flanhip_debug_kernel_scratch_bytes(int which);

/* ---- PV frame processors ------------------------------------------------------------------------------------- */
/* modify_time_base (PV/PVModify.cpp:307-362, linear Interpolator): mod_seconds is the sampled time map float[F][bins]
 * (FunctionSample2d layout, FunctionSample.h:173-199).  out: MF[ch][out_frames][bins], out_frames from
 * flanhip_modify_time_out_frames(). */
int flanhip_modify_time(const flanhip_MF * pv, int64_t num_channels, int64_t num_pv_frames, int num_bins,
                        float sample_rate, int hop, const float * mod_seconds,
                        int64_t out_frames, flanhip_MF * out, volatile int * cancel);
int flanhip_modify_time_dev(const flanhip_MF * d_pv, int64_t num_channels, int64_t num_pv_frames, int num_bins,
                            float sample_rate, int hop, const float * d_mod_seconds,
                            int64_t out_frames, flanhip_MF * d_out, void * stream);
/* PV::stretch front half (PV/PVModify.cpp:371-382): in-place inclusive prefix sum over frames per bin (fp32, sequential
 * order) then frame_to_time.  d_factor: float[F][bins] factor grid in, seconds out; flanhip_stretch_map_dev (below) also
 * reduces the maximum of the result into *d_max (float) when that pointer is given. */
/* modify_time for a PV that goes on to convert_to_audio: d_workspace is a synthesis workspace for the OUTPUT PV
 * (flanhip_synthesize_workspace_bytes( ch, out_frames, bins, sr, analysis_rate, window_size ); hop = int( sr / analysis_rate )).  When the time map never runs
 * backwards (every stretch) the kernel that writes the output also leaves convert_to_audio's pre-pass there;
 * flanhip_synthesize_dev_fused_checked then skips its own.  Same output as flanhip_modify_time_dev in every case. */
int flanhip_modify_time_dev_fused(const flanhip_MF * d_pv, int64_t num_channels, int64_t num_pv_frames, int num_bins,
                                  float sample_rate, float analysis_rate, const float * d_mod, int64_t out_frames,
                                  flanhip_MF * d_out, int window_size, void * d_workspace, void * stream);
int flanhip_stretch_map_dev(float * d_factor, int64_t num_pv_frames, int num_bins, float sample_rate, int hop,
                            float * d_max, void * stream);
/* PV::stretch with a CONSTANT factor: the whole map (running sum down the frames + frame_to_time, and its maximum) from the factor alone -- the sum
 * of a constant has a closed form that reproduces the sequential fp32 additions bit for bit (flan_amd/csrc/const_sum.h), so nothing is filled and
 * nothing is scanned.  d_map: float[F][bins] out.  Same result as flanhip_fill_dev + flanhip_stretch_map_dev. */
int flanhip_stretch_map_const_dev(float factor, float * d_map, int64_t num_pv_frames, int num_bins, float sample_rate, int hop,
                                  float * d_max, void * stream);
/* A grid filled with one value on the device (a constant-valued Function, sampled: `[](TF){ return c; }`). */
int flanhip_fill_dev(float * d_grid, int64_t count, float value, void * stream);

/* modify_frequency_base (PV/PVModify.cpp:196-257): mod_hz float[F][bins] = where each grid bin centre maps;
 * in_modified float[ch][F][bins] = new frequency of every MF.  out: MF[ch][F][bins]. */
int flanhip_modify_frequency(const flanhip_MF * pv, int64_t num_channels, int64_t num_pv_frames, int num_bins,
                             float sample_rate, const float * mod_hz, const float * in_modified,
                             flanhip_MF * out, volatile int * cancel);
int flanhip_modify_frequency_dev(const flanhip_MF * d_pv, int64_t num_channels, int64_t num_pv_frames, int num_bins,
                                 float sample_rate, const float * d_mod_hz, const float * d_in_modified,
                                 flanhip_MF * d_out, void * stream);
/* PV::repitch front half (PV/PVModify.cpp:273-302): d_factor float[F][bins] factor grid in -> Hz map out;
 * d_in_modified float[ch][F][bins] out. */
int flanhip_repitch_map_dev(const flanhip_MF * d_pv, int64_t num_channels, int64_t num_pv_frames, int num_bins,
                            float sample_rate, float * d_factor, float * d_in_modified, void * stream);
/* PV::repitch in one piece (PV/PVModify.cpp:273-305): d_factor float[F][bins] is turned into the Hz map in place (the running sum
 * over bins, :278-284) and modify_frequency_base runs with every MF's target frequency looked up on the fly (:289-302) -- the
 * same results as flanhip_repitch_map_dev + flanhip_modify_frequency_dev without the intermediate float[ch][F][bins] grid. */
int flanhip_repitch_dev(const flanhip_MF * d_pv, int64_t num_channels, int64_t num_pv_frames, int num_bins, float sample_rate,
                        float * d_factor, flanhip_MF * d_out, void * stream);
/* The same four with a named non-linear Interpolator (PVModify.cpp:232 and :344 apply interp( ... ) to the mixing coordinate of every
 * output bin / frame; Utility/Interpolator.cpp:14-101).  interp: FLANHIP_INTERP_* (below); FLANHIP_INTERP_LINEAR gives the plain calls
 * bit for bit. */
int flanhip_modify_time_interp_dev(const flanhip_MF * d_pv, int64_t num_channels, int64_t num_pv_frames, int num_bins,
                                   float sample_rate, int hop, const float * d_mod_seconds,
                                   int64_t out_frames, int interp, flanhip_MF * d_out, void * stream);
int flanhip_modify_time_interp_dev_fused(const flanhip_MF * d_pv, int64_t num_channels, int64_t num_pv_frames, int num_bins,
                                         float sample_rate, float analysis_rate, const float * d_mod_seconds,
                                         int64_t out_frames, int interp, flanhip_MF * d_out, int window_size, void * d_synth_workspace, void * stream);
int flanhip_modify_frequency_interp_dev(const flanhip_MF * d_pv, int64_t num_channels, int64_t num_pv_frames, int num_bins,
                                        float sample_rate, const float * d_mod_hz, const float * d_in_modified,
                                        int interp, flanhip_MF * d_out, void * stream);
int flanhip_repitch_interp_dev(const flanhip_MF * d_pv, int64_t num_channels, int64_t num_pv_frames, int num_bins, float sample_rate,
                               float * d_factor, int interp, flanhip_MF * d_out, void * stream);


/* PV::shape (PV/PV.cpp:421-458) for the affine shaper  mf -> { a*m + b, c*f + d }; arbitrary host callables are
 * evaluated by the C++ layer on the host grid and uploaded through flanhip_shape_table_dev. */
int flanhip_shape_affine(const flanhip_MF * pv, int64_t num_channels, int64_t num_pv_frames, int num_bins,
                         float sample_rate, float a, float b, float c, float d, int use_shift_alignment,
                         flanhip_MF * out, volatile int * cancel);
int flanhip_shape_affine_dev(const flanhip_MF * d_pv, int64_t num_channels, int64_t num_pv_frames, int num_bins,
                             float sample_rate, float a, float b, float c, float d, int use_shift_alignment,
                             flanhip_MF * d_out, void * stream);
/* Same placement rule with the shaped values precomputed (d_shaped: MF[ch][F][bins] = shaper(in) per MF). */
int flanhip_shape_table_dev(const flanhip_MF * d_pv, const flanhip_MF * d_shaped, int64_t num_channels,
                            int64_t num_pv_frames, int num_bins, float sample_rate, int use_shift_alignment,
                            flanhip_MF * d_out, void * stream);
/* The same without shift alignment, leaving PV::convert_to_audio's pre-pass for the RESULT in a synthesis workspace (d_ws of
 * flanhip_synthesize_workspace_bytes for the result's shape): follow with flanhip_synthesize_dev_fused on d_out. */
int flanhip_shape_affine_dev_fused(const flanhip_MF * d_pv, int64_t num_channels, int64_t num_frames, int num_bins, float sample_rate,
                                   float analysis_rate, float a, float b, float c, float d, flanhip_MF * d_out, int window_size,
                                   void * d_ws, void * stream);
int flanhip_shape_table_dev_fused(const flanhip_MF * d_pv, const flanhip_MF * d_shaped, int64_t num_channels, int64_t num_frames,
                                  int num_bins, float sample_rate, float analysis_rate, flanhip_MF * d_out, int window_size,
                                  void * d_ws, void * stream);

/* ---- further PV frame processors.  User functions are SAMPLED BY THE CALLER, as the reference samples
 * them on the host before its loops (PV.h:31-35, Function.h:141-171): a grid pointer, or NULL plus a constant. ------------- */

/* Utility/Interpolator.cpp:14-101: the named interpolators a device kernel can evaluate itself */
#define FLANHIP_INTERP_LINEAR        0
#define FLANHIP_INTERP_MIDPOINT      1
#define FLANHIP_INTERP_NEAREST       2
#define FLANHIP_INTERP_FLOOR         3
#define FLANHIP_INTERP_CEIL          4
#define FLANHIP_INTERP_SMOOTHSTEP    5
#define FLANHIP_INTERP_SMOOTHERSTEP  6
#define FLANHIP_INTERP_SQRT          7
#define FLANHIP_INTERP_SINE          8   /* cosf based: agrees with the host libm to 1-2 ulp, not bit for bit */
/* An Interpolator built from an arbitrary callable (Utility/Interpolator.h: Interpolator( std::function<float(float)> )): the caller samples it
 * at i / FLANHIP_INTERP_TABLE_INTERVALS, i = 0 .. INTERVALS, plus its value at NaN (INTERVALS + 2 floats, host memory), and gets a kind
 * (>= FLANHIP_INTERP_TABLE_FIRST, at most 32 alive per process) that every entry point taking FLANHIP_INTERP_* accepts ON THE DEVICE THAT WAS
 * CURRENT AT CREATION -- on another device the kind is rejected as unknown (create one table per device).  The kernels read the
 * table with linear interpolation between neighbouring samples, argument clamped to [0, 1]: exact at the sample points, within
 * max|f''| / ( 8 INTERVALS^2 ) = 2.9e-11 max|f''| between them -- below one fp32 step for any smooth shaping curve; a jump of the callable is
 * smeared over one interval (1.5e-5 wide).  _destroy synchronises the table's own device before the table is freed, whichever device is current. */
#define FLANHIP_INTERP_TABLE_INTERVALS 65536
#define FLANHIP_INTERP_TABLE_FIRST     16
int flanhip_interp_table_create(const float * samples, int * kind);
int flanhip_interp_table_destroy(int kind);

/* PV::replace_amplitudes (PV/PV.cpp:205-236): out = { src.m * a + m * (1-a), f }, a = clamp(amount,0,1), on the overlap of the
 * two PVs; zero elsewhere.  d_amount: float[F][bins] over THIS pv's domain, or NULL to use amount_const. */
int flanhip_replace_amplitudes_dev(const flanhip_MF * d_pv, int64_t num_channels, int64_t num_frames, int num_bins,
                                   const flanhip_MF * d_src, int64_t src_channels, int64_t src_frames, int src_bins,
                                   const float * d_amount, float amount_const, flanhip_MF * d_out, void * stream);
/* PV::subtract_amplitudes (PV/PV.cpp:238-264): out = copy, m = |m - src.m * amount| on the overlap (amount not clamped) */
int flanhip_subtract_amplitudes_dev(const flanhip_MF * d_pv, int64_t num_channels, int64_t num_frames, int num_bins,
                                    const flanhip_MF * d_src, int64_t src_channels, int64_t src_frames, int src_bins,
                                    const float * d_amount, float amount_const, flanhip_MF * d_out, void * stream);

/* PV::resonate (PV/PV.cpp:604-641).  Output frames (:613) = num_frames + ceil( time_to_frame( max(length,0) ) ). */
int64_t flanhip_resonate_out_frames(int64_t num_frames, float length_seconds, float sample_rate, int hop);
/* d_decay: float[out_frames][bins] sampled over the OUTPUT's domain (:616), or NULL to use decay_const; clamped to [0,1] (:617).
 * The per-frame factor pow(decay, seconds per frame) (:631) is the host libm's powf for a constant (bit for bit the
 * reference's call on this platform) and the correctly rounded power for a grid. */
int flanhip_resonate_dev(const flanhip_MF * d_pv, int64_t num_channels, int64_t num_frames, int num_bins, float sample_rate, int hop,
                         int64_t out_frames, const float * d_decay, float decay_const, flanhip_MF * d_out, void * stream);

/* PV::retain_n_loudest_partials / remove_n_loudest_partials (PV/PV.cpp:552-602).  d_n: int32[num_frames], the sampled
 * Function<Second,Bin> (:555), or NULL to use n_const; clamped to [0, num_frames] as the reference does (:556).
 * Bins of equal |m| rank by ascending bin (the reference's std::sort leaves their order unspecified). */
int flanhip_n_loudest_partials_dev(const flanhip_MF * d_pv, int64_t num_channels, int64_t num_frames, int num_bins,
                                   const int32_t * d_n, int32_t n_const, int remove, flanhip_MF * d_out, void * stream);

/* PV::desample (PV/PVModify.cpp:445-511).  d_ratio: float[F][bins] or NULL + ratio_const; interp: FLANHIP_INTERP_* */
int flanhip_desample_dev(const flanhip_MF * d_pv, int64_t num_channels, int64_t num_frames, int num_bins,
                         const float * d_ratio, float ratio_const, int interp, flanhip_MF * d_out, void * stream);

/* PV::time_extrapolate (PV/PVModify.cpp:607-666) after its input validation: 0 <= start_frame < end_frame < num_frames,
 * out_frames = end_frame + extrapolated frames (:627), d_interp_samples: float[out_frames - start_frame] sampled by the caller
 * as :631-633 does.  d_out: MF[ch][out_frames][bins]. */
int flanhip_time_extrapolate_dev(const flanhip_MF * d_pv, int64_t num_channels, int64_t num_frames, int num_bins, float sample_rate,
                                 int64_t start_frame, int64_t end_frame, int64_t out_frames, const float * d_interp_samples,
                                 flanhip_MF * d_out, void * stream);

/* ---- PV methods that select, rearrange and re-place frames and bins (PV/PV.cpp:24-39, :92-198, :362-419, :643-720) ---- */
/* PV::get_frame (PV/PV.cpp:24-39): one frame interpolated between its neighbours (getBinInterpolated, :62-73).
 * frame_pos = clamp( time_to_frame( time ), 0, F-1 ) is the caller's (:28); d_out: MF[ch][1][bins]. */
int flanhip_get_frame_dev(const flanhip_MF * d_pv, int64_t num_channels, int64_t num_frames, int num_bins, float frame_pos,
                          int interp, flanhip_MF * d_out, void * stream);
/* out[c][o][:] = pv[c][src[o]][:], zero where src[o] < 0: the copy loops of PV::freeze (PV/PV.cpp:176-195).
 * d_src_frames: int32[out_frames] (flanhip_freeze_plan fills the host copy). */
int flanhip_select_frames_dev(const flanhip_MF * d_pv, int64_t num_channels, int64_t num_frames, int num_bins,
                              const int32_t * d_src_frames, int64_t out_frames, flanhip_MF * d_out, void * stream);
/* PV::freeze's timing logic (PV/PV.cpp:140-171), host arithmetic: the output's frame count (returned; -1 on bad arguments) and,
 * when src_frames is not NULL, the input frame every output frame repeats (-1: stays zero).  times / lengths: n pairs, seconds.
 * Of several events on one frame the first given survives (unspecified in the reference: its sort is not stable). */
int64_t flanhip_freeze_plan(int64_t num_frames, float sample_rate, int hop, const float * times, const float * lengths, int n,
                            int32_t * src_frames);
/* PV::cut_frames (PV/PV.cpp:643-668): its input validation (count 0 = the null PV it returns), and the copy. */
int flanhip_cut_frames_range(int64_t num_frames, int32_t start, int32_t end, int32_t * start_out, int32_t * count_out);
int flanhip_cut_frames_dev(const flanhip_MF * d_pv, int64_t num_channels, int64_t num_frames, int num_bins, int64_t start,
                           int64_t count, flanhip_MF * d_out, void * stream);
/* one input of PV::join (PV/PV.cpp:708-716): its frames to out frames [out_start, out_start + in_frames), the channels and bins
 * both have; the caller clears d_out first (:706) */
int flanhip_place_frames_dev(const flanhip_MF * d_in, int64_t in_channels, int64_t in_frames, int in_bins, flanhip_MF * d_out,
                             int64_t out_channels, int64_t out_frames, int out_bins, int64_t out_start, void * stream);
/* PV::select (PV/PV.cpp:92-127).  d_selector_tf: TF{ t, f }[out_frames][bins], the selector sampled over the OUTPUT's domain
 * (:103); out_frames = Frame( time_to_frame( length ) ) (:101).  d_out: MF[ch][out_frames][bins]. */
int flanhip_select_dev(const flanhip_MF * d_pv, int64_t num_channels, int64_t num_frames, int num_bins, float sample_rate, int hop,
                       const float * d_selector_tf, int64_t out_frames, flanhip_MF * d_out, void * stream);
/* PV::add_octaves (mode 0) / PV::add_harmonics (mode 1) (PV/PV.cpp:362-419).  d_series: float[F][num_harmonics], the series
 * callable at ( frame_to_time( frame ), harmonic ) for the 0-based harmonic index, as :371-379 samples it; num_harmonics =
 * ceil( log2( get_height() ) ) for octaves (:412), num_bins for harmonics (:418).  dft sizes up to 8192. */
int flanhip_harmonic_scale_dev(const flanhip_MF * d_pv, int64_t num_channels, int64_t num_frames, int num_bins, float sample_rate,
                               const float * d_series, int num_harmonics, int mode, flanhip_MF * d_out, void * stream);

/* PV::modify (PV/PVModify.cpp:15-193): the general time / frequency warp.  The caller samples the callable twice, as the
 * reference does:  d_mod_tf: TF{ t, f }[F][bins], mod over the input's grid (:22), seconds / Hz;  d_in_f: float[ch][F][bins],
 * mod( { frame_to_time( frame ), the MF's own frequency } ).f (:62-66).  interp: FLANHIP_INTERP_*.
 * flanhip_modify_out_frames (host arithmetic, host grid): the output's frame count (:28-38); -2 when it would be longer than 10
 * minutes (the reference prints a message and returns a null PV, :30-34), 0 when there is nothing to make, -1 on bad arguments.
 * Equally loud candidates for an output point: the first input quad in ( frame, bin ) order gives the frequency (unspecified in the
 * reference, which runs frames in parallel); quads with a non-finite corner offer nothing. */
int64_t flanhip_modify_out_frames(const float * mod_tf, int64_t num_frames, int num_bins, float sample_rate, int hop);
int flanhip_modify_dev(const flanhip_MF * d_pv, int64_t num_channels, int64_t num_frames, int num_bins, float sample_rate, int hop,
                       const float * d_mod_tf, const float * d_in_f, int interp, int64_t out_frames, flanhip_MF * d_out, void * stream);

/* PV::stretch_spline (PV/PVModify.cpp:387-443; the spline is the reference's vendored spline/spline.h:284-401, fp64).
 * steps: HOST uint32[F-1], safeInterpolation( frame ) = max( uint32( interpolation( frame * frame_to_time( 1 ) ) ), 1 ) of every
 * frame but the last (:391-394); the output has sum( steps ) frames (:399-405, flanhip_stretch_spline_out_frames; -1 when F < 3,
 * a step is 0 or the sum does not fit a Frame).  Allocates its workspace (8 B x F x ch x bins x 2) from the stream's memory pool. */
int64_t flanhip_stretch_spline_out_frames(const uint32_t * steps, int64_t num_frames);
int flanhip_stretch_spline_dev(const flanhip_MF * d_pv, int64_t num_channels, int64_t num_frames, int num_bins,
                               const uint32_t * steps, int64_t out_frames, flanhip_MF * d_out, void * stream);

/* PV::smear_time (PV/PVModify.cpp:513-605).  The caller samples the three callables as :520-524 and :558-560 do:
 *   smear: float[F][bins] seconds (NULL: smear_const), clamped to >= 0 inside;  granularity: int32[F][bins] (NULL: the constant),
 *   clamped to >= 1 inside;  distribution: float[2 * dist_samples_2], distribution( x / dist_samples_2 ), x in [-dist_samples_2, dist_samples_2).
 * flanhip_smear_time_plan (host arithmetic, host grid): the frame the output starts at, its frame count (:563) and dist_samples_2 (:555-556). */
int flanhip_smear_time_plan(int64_t num_frames, int num_bins, float sample_rate, int hop, const float * smear, float smear_const,
                            int32_t * true_left, int64_t * out_frames, int32_t * dist_samples_2);
int flanhip_smear_time_dev(const flanhip_MF * d_pv, int64_t num_channels, int64_t num_frames, int num_bins, float sample_rate, int hop,
                           const float * d_smear, float smear_const, const int32_t * d_granularity, int32_t granularity_const,
                           const float * d_distribution, int64_t n_distribution, int32_t true_left, int64_t out_frames,
                           flanhip_MF * d_out, void * stream);

/* ---- Audio::convert_to_mid_side / convert_to_left_right (Audio/AudioConversions.cpp:32-56), stereo only ------ */
int flanhip_mid_side_dev(const float * d_in, int64_t num_audio_frames, float * d_out, void * stream);

/* ---- Audio::convert_to_SPV / SPV::convert_to_audio: the sliding-DFT vocoder (Conversions/AudioSPV.cpp, SPV/SPVBuffer.cpp) --- */
/* N = num_bins (the reference's dft_size), L = 2 N.  audio: float[ch][n]; spv: flanhip_MF[ch][n][N] -- one spectrum per input sample,
 * so 8 n N bytes per channel (1 s of 48 kHz at N = 1024: 393 MB).  The analysis rate of an SPV is its sample rate and bin b sits at
 * b sr / N (SPVBuffer.cpp).  Analysis (AudioSPV.cpp:27-108): L-point sliding DFT of the trailing window, frequency-domain Hann 3-tap
 * (with the reference's edge rule at bins 0 and N-1), phase_vocoder with the phases of the previous SAMPLE.  The GPU seeds each chain
 * of frames from a direct sum over the window before it, so the spectra follow the exact transform more closely than
 * the reference's fp32 running sum over the whole channel; they are not bit-identical to it.  Synthesis (AudioSPV.cpp:110-145):
 * inverse_phase_vocoder per bin, sample = 2 sum_b (-1)^b m cos( phase ).
 * Differences from the reference, on purpose: indices are 64-bit, so the twiddle index (f b) mod L is the intended one past
 * f b >= 2^31 (the reference's int32 product turns negative there, about 44.7 s at 48 kHz and N = 1024, and indexes out of its
 * table); N < 2 is FLANHIP_ERR_UNSUPPORTED (the reference reads bin 1 of a one-bin frame).  N up to 2^24.
 * `cancel` is polled before the upload and before the launch.  Unlike the STFT kernels, the SPV kernels do not poll it: once launched they
 * run to the end, and a flag raised meanwhile makes the call return FLANHIP_ERR_CANCELLED after the stream has drained. */
int flanhip_spv_analyze(const float * audio, int64_t num_channels, int64_t num_audio_frames, float sample_rate, int num_bins,
                        flanhip_MF * out, volatile int * cancel);
int flanhip_spv_analyze_dev(const float * d_audio, int64_t num_channels, int64_t num_audio_frames, float sample_rate, int num_bins,
                            flanhip_MF * d_out, void * stream);
/* bytes of device workspace flanhip_spv_synthesize_dev needs (pure host arithmetic; 0 for arguments it refuses).  Sized for the
 * calling thread's flanhip_spv_debug_chain_length setting: size and launch under the same one. */
size_t flanhip_spv_synthesize_workspace_bytes(int64_t num_channels, int64_t num_frames, int num_bins, float sample_rate);
/* spv: flanhip_MF[ch][n][N]; out: float[ch][n] */
int flanhip_spv_synthesize(const flanhip_MF * spv, int64_t num_channels, int64_t num_frames, int num_bins, float sample_rate,
                           float * out, volatile int * cancel);
int flanhip_spv_synthesize_dev(const flanhip_MF * d_spv, int64_t num_channels, int64_t num_frames, int num_bins, float sample_rate,
                               float * d_out, void * d_workspace, void * stream);
/* SPV::modify_frequency / repitch (SPV/SPV.cpp:21-44) with a constant Function: f = value (multiply 0) or f = f * value (multiply 1),
 * m unchanged.  d_out may be d_spv. */
int flanhip_spv_modify_frequency_const_dev(const flanhip_MF * d_spv, int64_t num_channels, int64_t num_frames, int num_bins, float value,
                                           int multiply, flanhip_MF * d_out, void * stream);
/* the twiddle table T[i] = polar( 1.0f, omega i ), omega = -pi2 / L as a float (AudioSPV.cpp:13-22): float[2 L] (re, im).  No device. */
int flanhip_spv_twiddles(int num_bins, float * out);
/* test hook: frames per chain of the calling thread's SPV launches (0: the library's choice).  Results do not depend on the cut beyond
 * rounding. */
void flanhip_spv_debug_chain_length(int frames);

/* ---- Audio::convolve: partitioned FFT convolution (Audio/AudioCombination.cpp:299-352) --------------------------------------- */
/* audio: float[ch][n]; ir: float[ir_ch][m], at the audio's sample rate (resampling an IR of another rate is the C++ layer's job,
 * Audio::convolve); out: float[ch][n + m] (n + m frames, as the reference's; the last one is 0 up to round-off).
 * out[c][t] = sum_k audio[c][t-k] ir[c % ir_ch][k]: IR channels are used cyclically.  Uniformly partitioned overlap-save with
 * partition P: K = ceil( m / P ) IR spectra, J = ceil( (n + m) / P ) input and output spectra, each a 2P-point fp32
 * FFT on the device; the library takes the smallest P of 512, 1024, 2048, 4096 with K <= 32, else 4096.  Numerics: fp32 throughout,
 * within about 5e-7 rms (relative) of the exact convolution, not bit-identical to FFTW's D = 2 pow2( max( n, m ) ) transform;
 * deterministic (no floating-point atomics: two calls agree bit for bit).
 * normalize != 0: out *= 1.0f / max |out|, the max over frames [0, end) with end = clamp( Frame( float(N) / sr * sr ), 0, N - 1 ),
 * N = n + m (AudioBuffer::get_max_sample_magnitude() with default arguments, in fp32), the reciprocal and product in fp32 like the
 * reference's modify_volume_in_place.  sample_rate serves only this range.  If that max is 0 the gain is +inf, as in the reference:
 * every sample becomes NaN (0 * inf) or +-inf.
 * Workspace: 8 (P+1) (2 ch J + min( ch, ir_ch ) K) + 8192 bytes (the X and Y spectra, the IR spectra of the IR channels used, and
 * 64 partial maxima of normalize, 128 bytes apart).
 * Non-positive sizes, null pointers, a non-positive sample rate and (for _dev) a null workspace are FLANHIP_ERR_INVALID_ARG.
 * `cancel` is polled before the upload and before the launch; the kernels run to the end once launched. */
int64_t flanhip_convolve_out_frames(int64_t num_frames, int64_t ir_frames);           /* n + m; 0 for non-positive sizes */
/* bytes of device workspace flanhip_convolve_dev needs (pure host arithmetic; 0 for arguments it refuses).  Sized for the calling
 * thread's flanhip_convolve_debug_partition setting: size and launch under the same one. */
size_t  flanhip_convolve_workspace_bytes(int64_t num_channels, int64_t num_frames, int64_t ir_channels, int64_t ir_frames);
int flanhip_convolve(const float * audio, int64_t num_channels, int64_t num_frames, const float * ir, int64_t ir_channels, int64_t ir_frames,
                     float sample_rate, int normalize, float * out, volatile int * cancel);
int flanhip_convolve_dev(const float * d_audio, int64_t num_channels, int64_t num_frames, const float * d_ir, int64_t ir_channels,
                         int64_t ir_frames, float sample_rate, int normalize, float * d_out, void * d_workspace, void * stream);
/* test hook: the partition P of the calling thread's convolutions (0: the library's choice).  A P other than a power of two from 128 to
 * 4096 makes the calls FLANHIP_ERR_UNSUPPORTED (workspace 0).  Results do not depend on P beyond rounding. */
void flanhip_convolve_debug_partition(int samples);

/* ---- Audio::repitch: variable-rate sinc resampling (Audio/AudioTemporal.cpp:236-299 over WDL_Resampler, WDL/resample.cpp) ------ */
/* (the family is flanhip_audio_repitch_*: flanhip_repitch_dev is PV::repitch, above.)
 * audio: float[ch][n]; inv_factors: float[count], one per granularity_frames input frames, ALREADY inverted and clamped by the caller
 * ( clamp( 1.0f / factor, 1.0f / 1000, 1000 ), AudioTemporal.cpp:246-249: the C++ layer's job, Audio::repitch ); out: float[ch][out_frames].
 * Block b of the reference's loop (:267-296) resamples at rate ratio = sr / ( sr * inv_factors[ floor( in_frame / float( g ) ) ] ) and
 * delivers g output frames.  The hand-over between blocks -- the fractional read position and the samples that stay buffered -- is
 * reproduced exactly by a host loop in fp64 (flanhip_audio_repitch_plan; one addition per output frame); the samples are computed on the
 * device, one 2 x 64-tap sum each (1 x 64 where the rates are "ideal", :1095-1141) against a Blackman-Harris x sinc table the kernel builds
 * per run of blocks with the same ( filtpos, oversize ) (:1157-1202).  Products are fp32, sums fp64 in tap order, as in the SincSample
 * templates (:106-257).  Within a block the read position is fma( j, ratio, fracpos ), not j additions.  Numerics: within a few fp32 ulps of
 * the reference; deterministic (two calls agree bit for bit).  Output frames past the last block stay 0; frames past
 * out_frames are dropped.  Any channel count (the reference hangs above 64, :1220).
 * quality: FLANHIP_REPITCH_SINC (SetMode( true, 0, true, 64 )), FLANHIP_REPITCH_UNINTERPOLATED (SetMode( false, 0, false ): in[ int( srcpos ) ]);
 * FLANHIP_REPITCH_LINEAR (a time-varying biquad across the whole stream, :1276-1292, :1529-1543) is FLANHIP_ERR_UNSUPPORTED: not built.
 * Null pointers, non-positive sizes, sample_rate <= 0, an unknown quality and a count smaller than the loop needs are
 * FLANHIP_ERR_INVALID_ARG, before any device call.  A call whose loop would run more than 2^22 blocks (56 bytes of record each, on the
 * host and in the workspace; 70 minutes of output at 1 ms blocks) or 2^33 additions is FLANHIP_ERR_UNSUPPORTED, before anything is
 * allocated for it beyond the records counted so far. */
#define FLANHIP_REPITCH_SINC 0
#define FLANHIP_REPITCH_LINEAR 1
#define FLANHIP_REPITCH_UNINTERPOLATED 2
/* AudioTemporal.cpp:252: ceil( accumulate( inv_factors ) * g ), the sum sequential in fp32 (FunctionSample.h:136-148), the product fp32; 0 for
 * arguments it refuses */
int64_t flanhip_audio_repitch_out_frames(const float * inv_factors, int64_t count, int64_t granularity_frames);
/* The block loop alone (host arithmetic, no device): returns the number of blocks (or a negative FLANHIP_ERR_*) and fills the first
 * `capacity` records of every array that is not null: the stream index of the resampler buffer's first sample (the stream: 31 zeros -- none
 * for UNINTERPOLATED --, the input, zeros), srcpos of the block's first output frame relative to it, the ratio, the table's filtpos /
 * oversize / ideal flag (:1095-1141, :1327-1328), the block's first output frame, and what ResamplePrepare asks for (:1241).  *out_frames:
 * flanhip_audio_repitch_out_frames. */
int64_t flanhip_audio_repitch_plan(int64_t num_frames, float sample_rate, const float * inv_factors, int64_t count, int64_t granularity_frames,
                                   int quality, int64_t capacity, int64_t * offsets, double * fracpos, double * ratio, double * filtpos,
                                   int32_t * oversize, int32_t * ideal, int64_t * first_out, int32_t * wanted, int64_t * out_frames);
/* How the SINC launch cuts that plan into runs (host arithmetic, no device; the launch's own planner, for tests that must know which path
 * a shape takes): a run is consecutive blocks that one workgroup computes from one coefficient table.  Returns the number of runs (0 for
 * UNINTERPOLATED, which has none) or a negative FLANHIP_ERR_* as the plan does, and fills the first `capacity` records of every array that is
 * not null: the run's first block and block count, and the stream window it stages in LDS, [win_start, win_start + win_len); win_len 0
 * means the window is too long to stage and every tap is read from global memory.  *channels_per_group / *groups (nullable): the channels
 * one workgroup walks and the groups per run for num_channels channels (the grid is runs x groups); both 0 where there are no runs. */
int64_t flanhip_audio_repitch_runs(int64_t num_frames, float sample_rate, const float * inv_factors, int64_t count, int64_t granularity_frames,
                                   int quality, int64_t num_channels, int64_t capacity, int64_t * first_block, int32_t * num_blocks,
                                   int64_t * win_start, int32_t * win_len, int32_t * channels_per_group, int64_t * groups);
/* bytes of device workspace flanhip_audio_repitch_dev needs (host arithmetic: it runs the plan; 0 for arguments it refuses): the window
 * factors (64 x 2080 doubles), 56 bytes per block and 40 per run */
size_t flanhip_audio_repitch_workspace_bytes(int64_t num_frames, float sample_rate, const float * inv_factors, int64_t count,
                                             int64_t granularity_frames, int quality);
/* `cancel` is polled before the upload and before the launch; the kernels run to the end once launched. */
int flanhip_audio_repitch(const float * audio, int64_t num_channels, int64_t num_frames, float sample_rate, const float * inv_factors,
                          int64_t count, int64_t granularity_frames, int quality, float * out, volatile int * cancel);
/* d_audio / d_out: device memory; inv_factors: HOST memory (the plan runs on the host).  The workspace need not be cleared.  The plan's
 * records go up before the launch and the stream is synchronised once for that. */
int flanhip_audio_repitch_dev(const float * d_audio, int64_t num_channels, int64_t num_frames, float sample_rate, const float * inv_factors,
                              int64_t count, int64_t granularity_frames, int quality, float * d_out, void * d_workspace, void * stream);

/* ---- Audio::compress: the dynamic range compressor (Audio/AudioVolume.cpp:190-278) as two scans ------------------------------ */
/* audio: float[ch][n]; sidechain: float[side_ch][side_n], the detector's input (pass the audio itself for the reference's null
 * sidechain_source, :207-208); out: float[ch][n], may be the audio; gain_out (may be NULL): float[n], the factor c every channel's
 * frame is multiplied by.  Each of the five parameters is a curve of n floats (the reference samples every Function once per frame,
 * :220-224) or, with a NULL curve, the scalar.  Everything is fp32, as in the reference:
 *   detector input  max( 0, max_c sidechain[c][f] ): the SIGNED sample, no abs (:211-215), so a frame whose samples are all negative
 *                   detects 0 and the audio passes unchanged; a NaN sample is never taken
 *   per frame       x_G = 20 log10( max( |x|, 1e-6 ) ), y_G = the gain computer's three branches as written (:229-238; with a knee
 *                   width of 0 the knee branch is never reached), x_L = x_G - y_G, alpha = exp( -1 / ( t sr ) ) (a time of 0 gives 0)
 *   peak detector   y_1 = max( x_L, a_R y_1 + ( 1 - a_R ) x_L ), y_L = a_A y_L + ( 1 - a_A ) y_1, both from 0 (:250-251, :258-259)
 *   output          c = pow( 10, -y_L / 20 ) once per frame (the reference recomputes it per channel), out = in * c
 * The reference's loop is sequential over all frames; here both recurrences run as scans (flan_amd/csrc/compress.hip):
 * every lane replays a run of frames with the reference's fp32 operations in its order, from a state carried in by an fp64 scan.
 * log10, exp and pow are the fp64 functions rounded to fp32 once.  Deterministic (two calls agree bit for bit); c does not depend on ch.
 * Where the reference has no defined behaviour: a sidechain shorter than the audio (it reads out of bounds there) is
 * FLANHIP_ERR_INVALID_ARG; a longer one is read up to n; its sample rate is not looked at.  Negative or NaN times and a ratio of 0 go
 * through the IEEE arithmetic as they come.
 * Null audio / sidechain / out (and, for _dev, workspace), non-positive sizes, sample_rate <= 0 and side_n < n are
 * FLANHIP_ERR_INVALID_ARG, before any device call.  The workspace need not be cleared.
 * `cancel` is polled before the upload and before the launch; the kernels run to the end once launched. */
/* bytes of device workspace flanhip_compress_dev needs (pure host arithmetic; 0 for arguments it refuses): five rows of n floats (n
 * rounded up to 4) and 56 bytes per block of 256 runs.  Sized for the calling thread's flanhip_compress_debug_run setting. */
size_t flanhip_compress_workspace_bytes(int64_t num_frames);
int flanhip_compress(const float * audio, int64_t num_channels, int64_t num_frames, float sample_rate,
                     const float * sidechain, int64_t side_channels, int64_t side_frames,
                     const float * threshold_curve, float threshold, const float * ratio_curve, float ratio,
                     const float * attack_curve, float attack, const float * release_curve, float release,
                     const float * knee_width_curve, float knee_width,
                     float * out, float * gain_out, volatile int * cancel);
int flanhip_compress_dev(const float * d_audio, int64_t num_channels, int64_t num_frames, float sample_rate,
                         const float * d_sidechain, int64_t side_channels, int64_t side_frames,
                         const float * d_threshold, float threshold, const float * d_ratio, float ratio,
                         const float * d_attack, float attack, const float * d_release, float release,
                         const float * d_knee_width, float knee_width,
                         float * d_out, float * d_gain_out, void * d_workspace, void * stream);
/* test hook: the frames one lane replays in the calling thread's compressions, 1 ... 64 (larger values are taken as 64; 0: the
 * library's choice, 16).  Results do not depend on it beyond rounding. */
void flanhip_compress_debug_run(int frames);

/* ---- Audio::modify_volume (Audio/AudioVolume.cpp:5-13, 32-44) and Audio::set_volume (:46-67) --------------------------------- */
/* out[c][f] = audio[c][f] * g[f], one fp32 product per sample, the same curve for every channel: d_gain is float[n] (the gain Function
 * sampled at f * ( 1.0f / sr ), :36) or NULL for the scalar `gain`.  d_out may be d_audio. */
int flanhip_audio_gain_dev(const float * d_audio, int64_t num_channels, int64_t num_frames, const float * d_gain, float gain,
                           float * d_out, void * stream);
/* out[c][f] = audio[c][f] * ( level[f] / m ): one fp32 division, then one fp32 product (:66).  m = get_max_sample_magnitude() with
 * default arguments (:63): the max |sample| over frames [0, end), end = clamp( Frame( float(N) / sr * sr ), 0, N - 1 ), so the LAST FRAME
 * IS NOT LOOKED AT (AudioBuffer.cpp:416-430; flanhip_convolve's normalize has the same range).  m == 0 hands the input through
 * unchanged (:65).  m is reduced and read on the device: no host round trip.  d_level: float[n] or NULL for the scalar `level`; d_out may
 * be d_audio.  Workspace: 8192 bytes (the maximum and up to 1024 partial maxima; need not be cleared). */
size_t flanhip_audio_set_volume_workspace_bytes(int64_t num_channels, int64_t num_frames);   /* 0 for arguments it refuses */
int flanhip_audio_set_volume_dev(const float * d_audio, int64_t num_channels, int64_t num_frames, float sample_rate,
                                 const float * d_level, float level, float * d_out, void * d_workspace, void * stream);

/* ---- Audio::filter_1pole_lowpass / _highpass (Audio/AudioFilter.cpp:327-387) and filter_1pole_repeat_low / _high (:280-324):
 * cascades of TPT sections with a per-frame cutoff, every section a scan --------------------------------------------------------- */
/* audio: float[ch][n]; out: float[ch][n], may be the audio; the cutoff is a curve of n floats (the reference samples the Function once
 * per frame, :119, :291, :342) or, with a NULL curve, the scalar.  Everything is fp32, one rounding per operation, in the reference's order:
 *   per frame        T_half = pi / sr (pi = acosf( -1 )), c = std::clamp( cutoff, 1, sr / 2 ) (two comparisons: a NaN stays NaN),
 *                    w = tan( T_half c ) / T_half, g = w T_half (:19-30, :57, :67, :120); shared by all channels and sections
 *   1-pole section   G = g / ( 1 + g ), v = G ( x - s ), lp = v + s, s = lp + v; taps lp | x - lp (:61-74), s from 0
 *   2-pole section   g1 = 2 R + g, d = 1 / ( 1 + 2 R g + g g ), hp = ( x - g1 s1 - s2 ) d, v1 = g hp, bp = v1 + s1, s1 = bp + v1,
 *                    v2 = g bp, lp = v2 + s2, s2 = lp + v2; taps lp | hp (:164-182), s1 and s2 from 0
 *   BUTTERWORTH      order N: for odd N a 1-pole section first, then floor( N / 2 ) 2-pole sections with R_i = -cos( theta_i ),
 *                    theta_i = delta i + pi / 2 + delta / 2, delta = 2 pi / ( 2 N ) (:32-44, :338-365); every section taps low (_LOW) or
 *                    high (_HIGH); section k reads section k - 1's output.  Order 0 is a copy of the input (:337).
 *   REPEAT           `order` identical 1-pole sections, all tapping low or all tapping high (:296-303).  Order 0 is SILENCE, not a copy:
 *                    the reference's loop never writes its zero-initialised output.
 * The reference's loop is sequential over all frames; here every section is a scan over the frames (flan_amd/csrc/filter.hip, DESIGN.md
 * 4.15): a section is an affine map of its state, every lane replays a run of frames with the reference's fp32 operations from a state
 * carried in by an fp64 scan (rounded to fp32 once).  tan (and the cosine of R_i) is the fp64 function rounded to fp32 once.
 * Deterministic (two calls agree bit for bit); a channel's output does not depend on the channels filtered with it.
 * order: 0 ... 65535 (the reference's uint16_t).  Null audio / out (and, for _dev, workspace), non-positive sizes, sample_rate <= 0, an
 * unknown kind and an order outside the range are FLANHIP_ERR_INVALID_ARG, before any device call.  The workspace need not be cleared.
 * `cancel` is polled before the upload and before the launch; the kernels run to the end once launched. */
#define FLANHIP_FILTER_BUTTERWORTH_LOW  0
#define FLANHIP_FILTER_BUTTERWORTH_HIGH 1
#define FLANHIP_FILTER_REPEAT_LOW       2
#define FLANHIP_FILTER_REPEAT_HIGH      3
/* bytes of device workspace flanhip_filter_1pole_dev needs (pure host arithmetic; 0 for arguments it refuses): the row g of n floats (n
 * rounded up to 4), then 48 bytes (a block's map, sized for a 2-pole section's six doubles) per channel and block of 256 runs, then 16
 * bytes (the state carried into the block) per channel and block: 4 * roundup( n, 4 ) + 64 * ch * ceil( n / ( 256 * run ) ).  Sized for the
 * calling thread's flanhip_filter_debug_run setting. */
size_t flanhip_filter_1pole_workspace_bytes(int64_t num_channels, int64_t num_frames);
int flanhip_filter_1pole(const float * audio, int64_t num_channels, int64_t num_frames, float sample_rate,
                         const float * cutoff_curve, float cutoff, int kind, int order,
                         float * out, volatile int * cancel);
int flanhip_filter_1pole_dev(const float * d_audio, int64_t num_channels, int64_t num_frames, float sample_rate,
                             const float * d_cutoff, float cutoff, int kind, int order,
                             float * d_out, void * d_workspace, void * stream);
/* test hook: the frames one lane replays in the calling thread's filters, 1 ... 64 (larger values are taken as 64; 0: the library's
 * choice, 16).  Results do not depend on it beyond rounding. */
void flanhip_filter_debug_run(int frames);

/* ---- Audio::filter_2pole_lowpass / _bandpass / _highpass / _notch (Audio/AudioFilter.cpp:520-624), filter_2pole_lowshelf / _bandshelf /
 * _highshelf (:631-758) and filter_1pole_lowshelf / _highshelf (:431-512): cascades of the same two TPT sections whose cutoff, damping
 * and output mix change every frame, every section a scan (flan_amd/csrc/filter.hip) ---------------------------- */
/* audio, out: float[ch][n].  cutoff, damping and gain are each a curve of n floats or, with a NULL curve, the scalar.  Damping is not
 * looked at by the 1-pole kinds, gain not by kinds 2 ... 5.  Everything is fp32, one rounding per operation, in the reference's order; each
 * transcendental (acos, cos, sin, sqrt, pow, hypot, tan) is the fp64 function of the fp32 argument rounded to fp32 once; complex products
 * and quotients are the textbook forms, ( ac - bd, ad + bc ) and ( ac + bd, bc - ad ) / ( cc + dd ).  T_half = pi / sr, amp( d ) =
 * pow( 10, d / 20 ), clamp( c ) = std::clamp( c, 1, sr / 2 ) by two comparisons, pole_i = ( cos theta_i, sin theta_i ) with
 * flanhip_filter_1pole's theta_i, and EVERY section prewarps its own cutoff without a clamp: g = ( tan( T_half w ) / T_half ) T_half.
 *   LOW, BAND, HIGH   per frame w = clamp( cutoff ), R = damping (NOT clamped), alpha = acos( R ) / N.  For odd N one state-variable
 *                     section ( w, cos( alpha ) ) FIRST; then per pole above the axis TWO sections, p1 = pole_i w scaler and p2 = pole_i w /
 *                     scaler, each with w_k = |p| and R_k = -Re( p ) / |p|; scaler = pow( R + sqrt( R R - 1 ), 1 / N ) (real) where R > 1,
 *                     else exp( -i alpha ).  Order N is N sections; all tap lp (LOW), bp 2 R_k (BAND) or hp (HIGH) (:520-582).
 *                     R > 1 at a frame makes alpha NaN: every ODD order puts out NaN from that frame on; even orders are fine.
 *   NOTCH             ( 0 + ( -band ) ) + audio per sample (:614-624); order 0 is therefore SILENCE.
 *   LOWSHELF, HIGHSHELF   M = amp( ( gain / 2 ) / ( 2 N ) ), M2 = M M, w = cutoff M (NOT clamped), R = damping, the sections of LOW; each puts out
 *                     ( lp / ( M2 M2 ) + b / M2 ) + hp (LOWSHELF) or ( lp + b M2 ) + ( hp M2 ) M2 (HIGHSHELF), b = bp 2 R_k (:709-758).
 *   BANDSHELF         M = amp( -gain / ( 2 N ) ), w = cutoff, R = damping M -- which can pass 1: odd orders then go NaN --, output
 *                     ( lp + b / M2 ) + hp (:726-740).
 *   1POLE_LOWSHELF, 1POLE_HIGHSHELF   the tilt (:431-488) of gain (LOW) or -gain (HIGH): M = amp( gain / ( 2 N ) ), w = M clamp( cutoff ); for
 *                     odd N a 1-pole section first, lp M + ( x - lp ) / M; then per pole a 2-pole section with R = Re( pole_i ) / w --
 *                     NEGATIVE and tiny: from order 2 on the reference is mildly unstable, and that is kept -- and output
 *                     ( lp / M2 + bp 2 R ) + hp M2.  Then every sample times amp( gain / 2 ), one fp32 product (:490-512).
 * Order 0 is a copy (NOTCH: silence; the 1-pole shelves: the copy times amp( gain / 2 )).  Deterministic (two calls agree bit for bit); a
 * channel's output does not depend on the channels filtered with it.  out may be the audio for every kind except NOTCH, which reads the
 * input after the cascade: flanhip_filter2_dev with d_out == d_audio and NOTCH is FLANHIP_ERR_INVALID_ARG.  Otherwise the refusals are
 * flanhip_filter_1pole's, before any device call; flanhip_filter_debug_run sets the run length here too. */
#define FLANHIP_FILTER2_1POLE_LOWSHELF  0   /* AudioFilter.cpp:431-500 */
#define FLANHIP_FILTER2_1POLE_HIGHSHELF 1   /* :502-512 */
#define FLANHIP_FILTER2_LOW             2   /* :520-592 */
#define FLANHIP_FILTER2_BAND            3   /* :594-602 */
#define FLANHIP_FILTER2_HIGH            4   /* :604-612 */
#define FLANHIP_FILTER2_NOTCH           5   /* :614-624 */
#define FLANHIP_FILTER2_LOWSHELF        6   /* :631-724 */
#define FLANHIP_FILTER2_BANDSHELF       7   /* :726-740 */
#define FLANHIP_FILTER2_HIGHSHELF       8   /* :742-758 */
/* bytes of device workspace flanhip_filter2_dev needs (pure host arithmetic; 0 for arguments it refuses): the rows g, R and m of one
 * section, n floats each (n rounded up to 4), rewritten for every section, then flanhip_filter_1pole's 64 bytes per channel and block:
 * 12 * roundup( n, 4 ) + 64 * ch * ceil( n / ( 256 * run ) ).  Need not be cleared. */
size_t flanhip_filter2_workspace_bytes(int64_t num_channels, int64_t num_frames);
int flanhip_filter2(const float * audio, int64_t num_channels, int64_t num_frames, float sample_rate,
                    const float * cutoff_curve, float cutoff, const float * damping_curve, float damping,
                    const float * gain_curve, float gain, int kind, int order,
                    float * out, volatile int * cancel);
int flanhip_filter2_dev(const float * d_audio, int64_t num_channels, int64_t num_frames, float sample_rate,
                        const float * d_cutoff, float cutoff, const float * d_damping, float damping,
                        const float * d_gain, float gain, int kind, int order,
                        float * d_out, void * d_workspace, void * stream);

/* ---- Audio::filter_comb (Audio/AudioFilter.cpp:988-1043): the feedback comb whose delay changes every frame, a linear recurrence over a
 * forest of frames resolved by pointer jumping (flan_amd/csrc/comb.hip) -------------------------------------------- */
/* audio, out: float[ch][n]; out may be the audio.  cutoff, feedback and wet_dry are each a curve of n floats (the reference samples each
 * Function once per frame, :1008-1011) or, with a NULL curve, the scalar.  Everything is fp32, one rounding per operation, in the reference's
 * order; f = invert ? -1 : 1 (:1006):
 *   per frame n      w = std::clamp( cutoff, 1, sr / 2 ) (two comparisons: a NaN stays NaN), delay = 1 / ( 2 w ), d = delay sr (an fp32
 *                    product, AudioBuffer.cpp:406-409), t = float( n ) - d, p = (int) t truncated TOWARD ZERO (:1031-1032);
 *                    u_nmt = ( p < 0 || p >= n_frames ) ? 0 : u[p] (:1016-1020); shared by all channels
 *   state            u[n] = x[n] + ( k f ) u_nmt, k the feedback, NOT clamped (:1035)
 *   output           y[n] = a u[n] + ( ( 1 - a ) f ) u_nmt, a = wet_dry (:1038)
 * Kept: a t in ( -1, 0 ) truncates to 0 and reads u[0]; p == n (only n = 0 with d < 1) reads u[0] before it is written, which is 0; a
 * fractional d gives the delay n - trunc( n - d ); a NaN cutoff makes the cast undefined (INT_MIN on x86, which reads 0) and is DEFINED here
 * as no link.  So frame n hangs on frame p(n) if 0 <= p(n) < n and on nothing otherwise.
 * The reference's loop is sequential; here the links are followed by pointer jumping in fp64: with u[n] = X[n] + C[n] u[P[n]], from X = x,
 * C = k f, P = p, a round does X[n] += C[n] X[q], C[n] *= C[q], P[n] = P[q] for q = P[n], and ceil( log2 n ) rounds leave X = u, exact to
 * about 1e-15; u is rounded to fp32 ONCE and the output line runs in the reference's fp32 operations.  The result is within 1 fp32 ulp of
 * the exact u, closer than the reference's own loop, and not bit-identical to it except where the feedback is 0 or no frame has a link.
 * Deterministic (two calls agree bit for bit); a channel's output does not depend on the channels filtered with it.  _dev reads nothing
 * back and does not synchronise: it launches every round it may need (a scalar cutoff: ceil( log2 ceil( n / max( trunc d, 1 ) ) ) + 1 of
 * them), and a round whose predecessor left no live link returns at once.  The first rounds, an odd number k of them up to 9, run
 * tile-local in LDS in one launch: a tile of 2048 frames owns the later ones and computes the earlier ones as a halo, which must hold the
 * 2^k - 1 nearest ancestors of every frame it owns: ( 2^k - 1 ) ceil( d ) frames with a scalar cutoff, as many rounds as 1024 frames of
 * halo allow.  With a cutoff curve, whose delays the host does not know, and from 2^24 frames on the level is not used.  A tile checks
 * its halo on the device; if one fails (only a forced count can), every round runs globally as if the launch had not been: the same bits
 * either way, one pass wasted.
 * Limits.  |feedback| <= 1 is the contract: C is a product of feedbacks along a path, and with |feedback| > 1 over more than about a
 * thousand links it overflows fp64 and inf * 0 gives NaN where the reference had overflowed already or, on silence, had stayed 0; above 1
 * results are promised only while that product stays in fp64's range.  Where the reference's u is not finite, u here is not finite
 * either, inf or NaN unspecified; frames that do not descend from such a frame are unaffected.
 * Null audio / out (and, for _dev, workspace), non-positive sizes and sample_rate <= 0 are FLANHIP_ERR_INVALID_ARG, before any device call;
 * num_frames >= 2^31 (the links are int32) or num_channels > 2^20 is FLANHIP_ERR_UNSUPPORTED.  `cancel` is polled before the upload, before
 * the first launch and between the rounds. */
/* bytes of device workspace flanhip_filter_comb_dev needs (pure host arithmetic; 0 for arguments it refuses): 64 int32 words (word r < 32
 * set: round r had live links to follow; word 32 set: a tile of the LDS level failed; word 33, left by the last launch: the rounds the
 * result went through), then the planes X[2][ch][n] of doubles, the rows C[2][n] of doubles and the rows P[2][n] of int32, a round
 * reading one of each pair and writing the other: 256 + 16 * ch * n + 24 * n.  Need not be cleared. */
size_t flanhip_filter_comb_workspace_bytes(int64_t num_channels, int64_t num_frames);
/* test and A/B hook: the rounds the calling thread's comb calls run tile-local in LDS first: 0 the library's choice, negative none,
 * positive that many (taken down to an odd number, 9 at most, behind a halo of 1024 frames).  No output bit depends on it. */
void flanhip_filter_comb_debug_local(int rounds);
int flanhip_filter_comb(const float * audio, int64_t num_channels, int64_t num_frames, float sample_rate,
                        const float * cutoff_curve, float cutoff, const float * feedback_curve, float feedback,
                        const float * wet_dry_curve, float wet_dry, int invert,
                        float * out, volatile int * cancel);
int flanhip_filter_comb_dev(const float * d_audio, int64_t num_channels, int64_t num_frames, float sample_rate,
                            const float * d_cutoff, float cutoff, const float * d_feedback, float feedback,
                            const float * d_wet_dry, float wet_dry, int invert,
                            float * d_out, void * d_workspace, void * stream);

/* ---- Audio::filter_1pole_multinotch (Audio/AudioFilter.cpp:802-885) and filter_2pole_multinotch (:887-986), use_saturator == false: an
 * all-pass cascade coupled through an instantaneous feedback path, a scan of dense D x D state-space systems that change every frame
 * (flan_amd/csrc/multinotch.hip) ------------------------------------------------------------------------------------ */
/* audio, out: float[ch][n]; out may be the audio.  cutoff, damping, feedback and wet_dry are each a curve of n floats (one value per
 * frame, as the reference samples or calls each Function, :813-815, :830-831, :912-915, :978) or, with a NULL curve, the scalar.  The
 * 1-pole kind does not look at damping.  inv = invert ? -1 : 1 (:816), T_half = pi / sr (pi = acosf( -1 ), :818).  Per frame, shared by
 * all channels: c = std::clamp( cutoff, 1, sr / 2 ) (two comparisons: a NaN stays NaN), w = tan( T_half c ) / T_half, g = w T_half
 * (:814, :829, :833; the sections are then run with use_prewarp == false), k = feedback, R = damping, a = wet_dry.  Per channel and frame:
 *   1POLE   G = ( g - 1 ) / ( g + 1 ), M = ( sum_{i < order} pow( G, i ) s[order-1-i] ) * ( 2 / ( 1 + g ) ) (:834-839),
 *           x_bar = ( x + inv k M ) / ( 1 - inv k pow( G, order ) ) (:867); x_bar then runs through the `order` 1-pole sections in turn
 *           (Gs = g / ( 1 + g ), v = Gs ( in - s ), lp = v + s, s = lp + v, :61-74), each putting out lp - ( in - lp ) (the mix { 1, -1 }, :874)
 *   2POLE   d = 1 / ( 1 + 2 R g + g g ), G = d ( 1 - 2 R g + g g ), M = sum_{i < order} pow( G, i ) ( g s2 - s1 )[order-1-i] (:934-939),
 *           x_bar = ( x + inv k 4 R d M ) / ( 1 - inv k pow( G, order ) ) (:967); the sections are the state-variable ones (:164-182) with
 *           the frame's g and R, each putting out ( lp - bp 2 R ) + hp (the mix { 1, -1, 1 }, :974)
 *   then    y_bar = inv * the last section's output, y = a x_bar + ( 1 - a ) y_bar (:876-878, :976-979); every state starts at 0.
 * The reference's arithmetic is kept: pow with an integer exponent is the DOUBLE function, so M += pow * s is a double product and a
 * double sum rounded to float at every term, and the denominator is a double, the quotient rounded to float once; everything else is
 * fp32, one rounding per operation, left to right (inv * k first, the 2-pole numerator ((((inv k) 4) R) d) M).  tan is the fp64 function of the fp32
 * product rounded to fp32 once; pow( G, order ) is the fp64 function; the powers of the sum are i fp64 products, i fp64 ulps from pow.
 * Damping and feedback are NOT clamped.
 * The reference's loop is sequential; here a frame is the linear map s' = A s + b x of the D = order (1POLE) or 2 order (2POLE) states,
 * runs of frames are reduced in fp64 to dense pairs ( A, r ) that a team of lanes holds by columns, the pairs are scanned, and every run
 * is REPLAYED with the operations above from a start state rounded to fp32 once.  Deterministic (two calls agree bit for bit); a
 * channel's output does not depend on the channels filtered with it.  _dev reads nothing back and does not synchronise.
 * Limits.  |feedback| < 1 is the stable range.  Outside it results are promised only while the products of the frames' matrices stay in
 * fp64's range.  Where the reference's output is not finite, the output here is not finite either, inf or NaN unspecified; a sample
 * that is not finite reaches no earlier frame and no other channel.
 * NOT offered: use_saturator == true (:842-864, :942-964), a Newton iteration on tanh per frame from the previous output, which is not
 * linear in the state and so no scan; and order == 0, where the reference reads an uninitialised y_bar.
 * Null audio / out (and, for _dev, workspace), non-positive sizes, sample_rate <= 0, an unknown kind and order <= 0 are
 * FLANHIP_ERR_INVALID_ARG; D > 16 (1POLE order > 16, 2POLE order > 8), num_channels > 2^20 and num_frames > 2^36 are
 * FLANHIP_ERR_UNSUPPORTED; all before any device call.  `cancel` is polled before the upload, before the first launch and between the launches. */
#define FLANHIP_MULTINOTCH_1POLE 0   /* AudioFilter.cpp:802-885 */
#define FLANHIP_MULTINOTCH_2POLE 1   /* :887-986 */
/* bytes of device workspace flanhip_multinotch_dev needs (pure host arithmetic; 0 for arguments it refuses).  With DP = 4, 8 or 16, the
 * least of them >= D, a block of 256 threads has 128 / DP teams of `run` frames each: the row of denominators (n doubles, n rounded up to
 * 4) and the rows g, R, inv k and a (floats), then per channel and block a total of ( DP + 1 ) DP doubles and a carried state of DP:
 * 24 * roundup( n, 4 ) + 8 * DP * ( DP + 2 ) * ch * ceil( n / ( ( 128 / DP ) * run ) ); run is 16 DP (a block is 2048 frames) unless the
 * calling thread's flanhip_multinotch_debug_run setting says otherwise.  Need not be cleared. */
size_t flanhip_multinotch_workspace_bytes(int64_t num_channels, int64_t num_frames, int kind, int order);
/* test hook: the frames one team reduces and replays in the calling thread's multinotch calls, 1 ... 64 (larger values are taken as 64;
 * 0: the library's choice, 16 DP = 64, 128 or 256).  Results do not depend on it beyond rounding. */
void flanhip_multinotch_debug_run(int frames);
int flanhip_multinotch(const float * audio, int64_t num_channels, int64_t num_frames, float sample_rate,
                       const float * cutoff_curve, float cutoff, const float * damping_curve, float damping,
                       const float * feedback_curve, float feedback, const float * wet_dry_curve, float wet_dry,
                       int kind, int order, int invert, float * out, volatile int * cancel);
int flanhip_multinotch_dev(const float * d_audio, int64_t num_channels, int64_t num_frames, float sample_rate,
                           const float * d_cutoff, float cutoff, const float * d_damping, float damping,
                           const float * d_feedback, float feedback, const float * d_wet_dry, float wet_dry,
                           int kind, int order, int invert, float * d_out, void * d_workspace, void * stream);

/* ---- hilbert_phase_diff_network (Audio/AudioFilter.cpp:1045-1160) and the single-sideband methods over it: Audio::halfband_modulate
 * (:1162-1186), the modulation of Audio::shift_frequency (:1188-1227) and Audio::halfband_multiply (:1229-1263).  The network is two
 * cascades of ten 1-pole all-pass sections with constant poles; a cascade is one linear system with a constant 10 x 10 lower-triangular
 * matrix, scanned over the frames in one pass (flan_amd/csrc/halfband.hip) ------------------------------------------ */
/* :1109-1150, phase_diff_network_pole_design( 20, 5, 22000 ): the poles in rad/s, computed in fp64 and each rounded to fp32.  `first` has
 * the poles of the FIRST output's cascade, the odd-indexed ones of the design (the reference returns them "backwards"), `second` the
 * even-indexed ones.  They do not depend on the sample rate.  Host only. */
void flanhip_halfband_poles(float first[10], float second[10]);
/* bytes of device workspace the three _dev calls below need (pure host arithmetic; 0 for arguments it refuses): 15 packed triangular
 * matrices of 55 doubles for each of four cascades, then per channel and block of 256 runs the four cascades' totals and carried states,
 * ten doubles each: 26400 + 640 * ch * ceil( n / ( 256 * run ) ); ch and n are the OUTPUT's.  Sized for the calling thread's
 * flanhip_halfband_debug_run setting.  Need not be cleared. */
size_t flanhip_halfband_workspace_bytes(int64_t num_channels, int64_t num_frames);
/* test hook: the frames one lane replays in the calling thread's halfband calls, 1 ... 64 (larger values are taken as 64; 0: the library's
 * choice, 16).  Results do not depend on it beyond rounding. */
void flanhip_halfband_debug_run(int frames);
/* :1045-1072, :1152-1160: audio, first, second: float[ch][n].  Per channel and frame the sample goes through a cascade's sections in order,
 * each process_sample_and_mix( x, p_i, { 1, -1 }, false ) (:61-80): NO prewarp and NO clamp, the pole in rad/s is w.  In fp32, one rounding
 * per operation: T_half = pi / sr (pi = acosf( -1 )), g = p_i T_half, G = g / ( 1 + g ), v = G ( x - s ), lp = v + s, s = lp + v,
 * y = lp - ( x - lp ), s from 0.  Every lane replays a run of frames with these operations from a state carried in by an fp64 scan (rounded
 * to fp32 once).  first or second may be the audio.  Deterministic (two calls agree bit for bit); a channel's output does not depend on the
 * channels beside it.  Null audio / outputs (and, for _dev, workspace), non-positive sizes and sample_rate <= 0 are
 * FLANHIP_ERR_INVALID_ARG, before any device call.  `cancel` is polled before the upload and before the launch. */
int flanhip_hilbert(const float * audio, int64_t num_channels, int64_t num_frames, float sample_rate,
                    float * first, float * second, volatile int * cancel);
int flanhip_hilbert_dev(const float * d_audio, int64_t num_channels, int64_t num_frames, float sample_rate,
                        float * d_first, float * d_second, void * d_workspace, void * stream);
/* :1162-1186: out[c][f] = first[c][f] * re[f] - second[c][f] * im[f], two fp32 products and one fp32 difference, no fused multiply-add;
 * the network's outputs never go to memory.  re and im are each a curve of n floats or, with a NULL curve, the scalar.  A non-NULL phase
 * curve (n floats, radians) stands for both: re = cos( phase ), im = sin( phase ), the fp64 functions of the fp32 phase rounded to fp32 once
 * (:1225, std::exp( complex( 0, phase ) )).  out may be the audio.  The refusals of flanhip_hilbert. */
int flanhip_halfband_modulate(const float * audio, int64_t num_channels, int64_t num_frames, float sample_rate,
                              const float * re_curve, float re, const float * im_curve, float im, const float * phase_curve,
                              float * out, volatile int * cancel);
int flanhip_halfband_modulate_dev(const float * d_audio, int64_t num_channels, int64_t num_frames, float sample_rate,
                                  const float * d_re, float re, const float * d_im, float im, const float * d_phase,
                                  float * d_out, void * d_workspace, void * stream);
/* :1242-1260: a: float[ch_a][n_a], b: float[ch_b][n_b], out: float[min ch][min n].  Each operand goes through the network with ITS OWN
 * sample rate; out[c][f] = a_first * b_first - a_second * b_second, as above, over the first min ch channels and min n frames of both (the
 * network is causal: later frames do not reach earlier ones).  Four cascades in the same four launches; none of their outputs goes to
 * memory.  The band-pass before the network (:1235-1240) is not part of this call: Audio::halfband_multiply runs it with
 * flanhip_filter_1pole_dev.  The refusals of flanhip_hilbert, for both operands. */
int flanhip_halfband_multiply(const float * a, int64_t channels_a, int64_t frames_a, float sample_rate_a,
                              const float * b, int64_t channels_b, int64_t frames_b, float sample_rate_b,
                              float * out, volatile int * cancel);
int flanhip_halfband_multiply_dev(const float * d_a, int64_t channels_a, int64_t frames_a, float sample_rate_a,
                                  const float * d_b, int64_t channels_b, int64_t frames_b, float sample_rate_b,
                                  float * d_out, void * d_workspace, void * stream);

/* ---- Audio::stereo_spatialize (Audio/AudioSpatial.cpp:88-281): a mono source moving in the plane, rendered per ear
 * (flan_amd/csrc/spatial.hip) ------------------------------------------------------------------------------------- */
/* head_ild (:116-131) and falloff (:104-114) for one ear or both.  audio: float[n], mono (any other num_channels is
 * FLANHIP_ERR_INVALID_ARG); lowpassed: float[n], the audio through filter_1pole_lowpass( 500, 1 ) (flanhip_filter_1pole_dev; the same
 * for both ears); positions: double[n][2], the source's ( x, y ) per frame after the speed limiter (:238-257), or NULL for the constant
 * ( position_x, position_y ); out: float[1 or 2][n], with FLANHIP_SPATIAL_BOTH the left ear first.  Per frame f and ear, in the
 * reference's types and order, one rounding per operation and no fused multiply-add:
 *   q     = int( ( f * ( 1.0f / sr ) ) * sr ) in fp32 -- the frame the reference's callables read the weight and the distance at
 *           (FunctionSample.h:130-133, :109): f, or for some f, f - 1
 *   rel   = positions[q] - ( 0, +- head_width / 2.0f ) in fp64, + for the left ear (:261-263)
 *   mix   = 0.5f + 0.5f * cosf( atan2f( float( rel.y ), float( rel.x ) ) - direct ), direct = +- 75.0f * pi2 / 360.0f (:120-122, :276-277)
 *   out   = ( lowpassed[f] * ( 1.0f - mix ) + audio[f] * mix ) * ( 1.0f / ( float( |rel| ) + 0.00001f ) ) (:129-130, :112)
 * atan2f and cosf are the device's.  Null audio / lowpassed / out, a non-positive size, sample_rate <= 0, a NaN head_width and an unknown
 * `ears` are FLANHIP_ERR_INVALID_ARG, before any device call. */
#define FLANHIP_SPATIAL_LEFT  1
#define FLANHIP_SPATIAL_RIGHT 2
#define FLANHIP_SPATIAL_BOTH  3
int flanhip_spatial_ear(const float * audio, const float * lowpassed, int64_t num_channels, int64_t num_frames, float sample_rate,
                        const double * positions, double position_x, double position_y, float head_width, int ears,
                        float * out, volatile int * cancel);
int flanhip_spatial_ear_dev(const float * d_audio, const float * d_lowpassed, int64_t num_channels, int64_t num_frames, float sample_rate,
                            const double * d_positions, double position_x, double position_y, float head_width, int ears,
                            float * d_out, void * stream);
/* head_itd for a source that stands still (:139-153): out[e][ Frame( frame + delays[e] ) ] = audio[e][frame], the index formed in fp32
 * as the reference forms it, everything else 0.  d_audio: float[ears][n]; delays and out_frames: HOST arrays, one per ear (the delay in
 * frames, time_to_frame( dist / 343 ), and the ear's output length Frame( n + delay )); d_out: float[ears][out_stride], each row zero
 * past what is written.  Where two frames land on one index (above 2^24 frames) the later one stays, as in the reference's loop. */
int flanhip_spatial_delay_dev(const float * d_audio, int64_t num_ears, int64_t num_frames, const float * delays, const int64_t * out_frames,
                              int64_t out_stride, float * d_out, void * stream);
/* head_itd for a moving source (:155-221): the reference feeds a WDL_Resampler (SetMode( true, 0, true, 32 ), SetFeedMode( true ))
 * 32 input frames per block at the rate sr -> sr * stretches[block], and every block delivers what the resampler can give: a number of
 * output frames that depends on the data.  The hand-over between blocks -- the fractional read position and the samples that stay
 * buffered -- is reproduced exactly by a host loop in fp64 (flanhip_spatial_itd_plan; one addition per output frame); the samples are
 * computed on the device, one 2 x 32-tap sum each (1 x 32 where the rates are "ideal", WDL/resample.cpp:1095-1141) against a
 * Blackman-Harris x sinc table the kernel builds per run of blocks with the same ( filtpos, oversize ).  Products are fp32, sums fp64 in
 * tap order; within a block the read position is fma( j, ratio, fracpos ), not j additions.  The reference never flushes the resampler:
 * the last 33 or so input frames are not heard.  Deterministic (two calls agree bit for bit).
 * count = ceil( n / 32 ) everywhere: any other count is FLANHIP_ERR_INVALID_ARG, like null pointers, non-positive sizes, sample_rate <= 0,
 * more than two ears and a stretch that is not a number or outside [1/16, 1024] (the method's own stay within ( 1/2, 343 ]).  More than
 * 2^22 blocks or 2^33 output frames per ear are FLANHIP_ERR_UNSUPPORTED. */
/* :159-186 from the source's distances (metres, fp64) at frames 0, 32, 64, ...: returns the output length ceil( time_to_frame(
 * max_needed_length ) ) with the reference's float / double mix (0 for n <= 32), or a negative FLANHIP_ERR_*; stretches (may be NULL):
 * double[count], 1 / ( 1 - change / 32 / 343 * sr ).  Host arithmetic. */
int64_t flanhip_spatial_itd_out_frames(int64_t num_frames, float sample_rate, const double * distances, int64_t count, double * stretches);
/* The block loop alone (host arithmetic, no device): returns the number of blocks (or a negative FLANHIP_ERR_*) and fills the first
 * `capacity` records of every array that is not null: the stream index of the resampler buffer's first sample (the stream: 15 zeros,
 * the input, zeros), srcpos of the block's first output frame relative to it, the ratio, the table's filtpos / oversize / ideal flag, the
 * block's first output frame, the frames it delivers, and the samples buffered while it runs (15 + 32 in the first block, then 66 at
 * most; 64 to 66 for the method's own stretches).  *total_out: the frames all blocks deliver together. */
int64_t flanhip_spatial_itd_plan(int64_t num_frames, float sample_rate, const double * stretches, int64_t count, int64_t capacity,
                                 int64_t * offsets, double * fracpos, double * ratio, double * filtpos, int32_t * oversize, int32_t * ideal,
                                 int64_t * first_out, int32_t * delivered, int32_t * buffered, int64_t * total_out);
/* bytes of device workspace flanhip_spatial_itd_dev needs (host arithmetic: it runs the plans; 0 for arguments it refuses): the window
 * factors (64 x 1040 doubles), 56 bytes per block of every ear and 64 per run.  stretches: double[ears][count]. */
size_t flanhip_spatial_itd_workspace_bytes(int64_t num_ears, int64_t num_frames, float sample_rate, const double * stretches, int64_t count);
/* audio: float[ears][n], each ear's own input; stretches: double[ears][count] and out_frames: int64[ears], both HOST memory (the plans run
 * on the host); out: float[ears][out_stride].  Ear e keeps output frames below out_frames[e] <= out_stride (:213-215); frames no block
 * reaches, and the rest of the row, are 0.  Both ears run in one launch and each is what it would be alone.  The workspace need not be
 * cleared; the records go up before the launch and the stream is synchronised once for that.  `cancel` is polled before the upload and
 * before the launch. */
int flanhip_spatial_itd(const float * audio, int64_t num_ears, int64_t num_frames, float sample_rate, const double * stretches, int64_t count,
                        const int64_t * out_frames, int64_t out_stride, float * out, volatile int * cancel);
int flanhip_spatial_itd_dev(const float * d_audio, int64_t num_ears, int64_t num_frames, float sample_rate, const double * stretches,
                            int64_t count, const int64_t * out_frames, int64_t out_stride, float * d_out, void * d_workspace, void * stream);

/* ---- Audio::pan_in_place (Audio/AudioSpatial.cpp:21-40), convert_to_stereo / convert_to_mono (Audio/AudioConversions.cpp:58-104),
 * combine_channels / split_channels (Audio/AudioChannels.cpp) ------------------------------------------------------------------- */
/* audio, out: float[2][n] (any other num_channels is FLANHIP_ERR_INVALID_ARG); out may be the audio.  pan: a curve of n floats in [-1, 1]
 * or, with a NULL curve, the scalar.  p = pan[f] / 2.0f + 0.5f; channel 0 times sine2( p ), channel 1 times sine2( 1.0f - p ), with
 * sine2( x ) = float( double( sqrtf( 2 ) ) * sin( double( pi / 4.0f * x ) ) ) (Utility/Interpolator.cpp:85-91: the unqualified sin is the
 * double one there).  One fp32 product per sample. */
int flanhip_audio_pan(const float * audio, int64_t num_channels, int64_t num_frames, const float * pan_curve, float pan,
                      float * out, volatile int * cancel);
int flanhip_audio_pan_dev(const float * d_audio, int64_t num_channels, int64_t num_frames, const float * d_pan, float pan,
                          float * d_out, void * stream);
/* :68-77: mono float[n] -> float[2][n], both channels s / sqrt( 2.0f ) */
int flanhip_audio_to_stereo_dev(const float * d_audio, int64_t num_frames, float * d_out, void * stream);
/* :87-104: float[ch][n] -> float[n], the channels added in order from 0.0f in fp32, the sum divided by float( ch ) */
int flanhip_audio_to_mono_dev(const float * d_audio, int64_t num_channels, int64_t num_frames, float * d_out, void * stream);
/* num_rows rows of src_frames floats, src_stride apart, copied to rows dst_stride apart; every destination row is dst_frames >=
 * src_frames long and zero behind the copy.  combine_channels copies each input's channels into its rows of the output this way,
 * split_channels each channel into a buffer of its own.  The buffers must not overlap. */
int flanhip_audio_copy_rows_dev(const float * d_src, int64_t src_stride, int64_t num_rows, int64_t src_frames,
                                float * d_dst, int64_t dst_stride, int64_t dst_frames, void * stream);

/* ---- Audio::get_local_wavelength(s), get_average_wavelength (Audio/AudioInformation.cpp:18-75, 138-265; DSPUtility.h:19-20,
 * DSPUtility.cpp:37-147, 149-185): the YIN pitch tracker (flan_amd/csrc/pitch.hip) ------------------------------------ */
/* x: ONE channel row of num_frames floats.  Analysis windows of `window` samples begin at start, start + hop, ... while frame + window <
 * end (:180-183); end == -1 means num_frames.  Per window, with n = window and h = n / 2:
 *   compute_d (:18-57)        d[tau] = sum_{i<h} ( x[i] - x[i+tau] )^2 for tau < h.  The reference gets it as p0 + p_tau - 2 r[tau] from two
 *                             fp32 FFTs; here it is the sum itself -- fp32 differences, fmaf, 32 terms chained in fp32, the chunks added in
 *                             fp64 --, rounded to fp32 once: every term is >= 0 and nothing cancels, so it is closer to the exact sum than
 *                             the reference is and NOT bit-identical to it
 *   compute_d_prime (:59-75)  d'[0] = 1; a running double sum of the fp32 d; d'[tau] = float( double( d[tau] ) * ( tau / sum ) ), 1 where
 *                             the sum is 0.  Silence and a constant give d' == 1 exactly
 *   find_valleys( d' ) with its defaults (DSPUtility.h:19-20, DSPUtility.cpp:55-147): interior points 1 ... h - 2; a point is a valley if
 *                             the first differing value on either side is greater (an edge reached over equal values disqualifies); of a
 *                             plateau (right - left > 2) only the point floor( ( right + left ) * 0.5 ) counts, with x = that mean and y
 *                             the plain value; otherwise ( x, y ) = parabolic_interpolation (:37-43) of -d' with y negated, in fp32,
 *                             operation by operation; ordered by x
 *   the selection (:149-165)  k = the first valley with float( minimum_wavelength ) < x (none: 0); lowest = the first minimum of y from k
 *                             on; best = the first valley from k on with y < lowest.y * 2, or ( 0, 0 ) if there is none -- which is what
 *                             happens when lowest.y <= 0, as on an exactly periodic signal: the reference's behaviour, kept --; the
 *                             result is best.x if best.y < absolute_cutoff, else 0
 * For the same d' bits flanhip_audio_yin_pick_dev gives the bits of the reference's arithmetic.  Deviation: a d' row that holds a NaN or
 * an infinity gives 0 (the reference's walk then depends on where they lie); rows are promised while |d'| stays far inside fp32's range
 * (d' <= h when it comes from compute_d_prime).
 * Every form refuses, with FLANHIP_ERR_INVALID_ARG and before any device call, null pointers, hop < 1, start < 0, end > num_frames (or
 * below -1), window < 1 and num_frames < 0; window > 16384 (a block keeps the window and its d' in LDS) is FLANHIP_ERR_UNSUPPORTED.  With
 * h < 3 no interior point exists: zeros, without a launch. */
/* the number of windows (pure host arithmetic); -1 for arguments the forms refuse as invalid */
int64_t flanhip_audio_local_wavelengths_count(int64_t num_frames, int64_t start, int64_t end, int64_t window, int64_t hop);
/* d_dprime: float[count][h], d' of every window */
int flanhip_audio_yin_dprime_dev(const float * d_x, int64_t num_frames, int64_t start, int64_t end, int64_t window, int64_t hop,
                                 float * d_dprime, void * stream);
/* d_dprime: float[count][h] -> d_out: float[count], valleys and selection.  h > 8192 is FLANHIP_ERR_UNSUPPORTED */
int flanhip_audio_yin_pick_dev(const float * d_dprime, int64_t count, int64_t h, float absolute_cutoff, int64_t minimum_wavelength,
                               float * d_out, void * stream);
/* bytes of device workspace flanhip_audio_local_wavelengths_dev asks for (pure host arithmetic; 0 for arguments it refuses): 16 for every
 * shape served today -- the fused launch keeps a window's d' in LDS and leaves nothing there; the block is reserved for windows beyond LDS */
size_t flanhip_audio_local_wavelengths_workspace_bytes(int64_t num_frames, int64_t start, int64_t end, int64_t window, int64_t hop);
/* d_out: float[count], the RAW per-window wavelengths (no continuity pass), both steps in one launch: bit-identical to
 * flanhip_audio_yin_dprime_dev followed by flanhip_audio_yin_pick_dev */
int flanhip_audio_local_wavelengths_dev(const float * d_x, int64_t num_frames, int64_t start, int64_t end, int64_t window, int64_t hop,
                                        float absolute_cutoff, int64_t minimum_wavelength, float * d_out, void * d_workspace, void * stream);
/* Audio::get_local_wavelength (:138-166): one window, d_window[0 .. window) -> d_out[0] */
int flanhip_audio_local_wavelength_dev(const float * d_window, int64_t window, float absolute_cutoff, int64_t minimum_wavelength,
                                       float * d_out, void * stream);
/* Audio::get_local_wavelengths (:168-229), host pointers: out float[count], the windows' wavelengths after the continuity pass.  Only the
 * frames the windows read are uploaded.  `cancel` is polled before the upload, before the launch, while it runs and before the continuity pass. */
int flanhip_audio_local_wavelengths(const float * x, int64_t num_frames, float sample_rate, int64_t start, int64_t end, int64_t window, int64_t hop,
                                    float absolute_cutoff, int64_t minimum_wavelength, float * out, volatile int * cancel);
/* The continuity pass (:190-226), host-only, in place, as written: minimum_num_hops = int( ( 0.1f * sample_rate ) / float( hop ) ); the
 * hops i + 1 with 1.95 < w[i+1] / w[i] < 2.05 (w[i] != 0) are collected first; for each, the doubling's length is counted while the ratio to
 * w[hop] stays in [.95, 1.05] (a 0 is counted and skipped: the `continue` goes to the loop's condition), up to minimum_num_hops + 1; a
 * longer one is a new note and ENDS the pass (the `break` leaves the loop over the hops), a shorter one is halved -- so later ratios are
 * taken against halved values.  hop < 1 or count < 0 is FLANHIP_ERR_INVALID_ARG. */
int flanhip_wavelength_continuity(float * w, int64_t count, float sample_rate, int64_t hop);
/* Audio::get_average_wavelength( locals, ... ) (:245-265) with mean_and_sd (DSPUtility.cpp:159-185), host-only, fp32 in order: -1 unless
 * more than min_active_ratio * count entries differ from -1; then the mean of the entries that differ from 0 (a -1 stays in), or -1 if
 * max_length_sigma != -1 and their standard deviation exceeds it.  No non-zero entry: mean and deviation are 0. */
int flanhip_average_wavelength(const float * locals, int64_t count, float min_active_ratio, float max_length_sigma, float * out);

/* ---- Audio::mix and the granular family over it: cut, join, texture, synthesize_grains, granulate, psola (Audio/AudioCombination.cpp:102-237,
 * Audio/AudioSynthesis.cpp:310-473, 572-638, Audio/AudioTemporal.cpp:190-234, Audio/AudioVolume.cpp:102-135, WindowFunctions.cpp:10-13)
 * (flan_amd/csrc/grains.hip) ----------------------------------------------------------------------------------------- */
/* An EVENT is one term of Audio::mix (AudioCombination.cpp:102-170): n frames of a source from its frame s, added to the output from
 * frame o on (o may be negative: what falls before frame 0 is not heard, :162), over the source's channels, times a gain.  A grain of
 * granulate / psola is an event cut in flight: sf and ef are the fades of cut_frames (AudioTemporal.cpp:207-234), FLANHIP_GRAIN_HANN
 * psola's window (AudioSynthesis.cpp:626).  The reference makes every grain an Audio and adds them one after another (:155-167); here
 * every output sample out[c][g] is the sum, from +0.0f and IN ASCENDING EVENT INDEX, one fp32 addition per term, of the events with
 * o <= g < o + n and c < channels -- the order of the reference's loop, whatever the events' start frames; a lone -0.0f comes out
 * +0.0f, as it does after clear_buffer() (:152).  A term, with i = g - o, every step rounded to fp32:
 *   v = src[c][s + i]
 *   i < sf:       v *= sqrtf( float( i ) / sf )                  (AudioVolume.cpp:123-127 with Interpolator::sqrt())
 *   i >= n - ef:  v *= sqrtf( float( n - 1 - i ) / ef )          (:128-132; sf + ef <= n, so the ramps never share a frame)
 *   Hann:         v *= hann( ( i * ( 1.0f / sample_rate ) ) / ( n / sample_rate ) ), the grain's own time over its own length
 *                 (sample_function_over_domain, Audio/Audio.h:37), hann( x ) = float( 0.5 * ( 1.0 - cos( double( 2.0f * pi * x ) ) ) ),
 *                 pi = acosf( -1.0f ): WindowFunctions.cpp:10-13, whose unqualified cos is the DOUBLE one, as sine2's sin above
 *   term = v * gain (the scalar, or gains[gain_offset + i]: the amplitude Function sampled over the event, AudioCombination.cpp:138)
 * Without the Hann flag the result is bit-identical to the reference's loop; with it the device's double cos may differ from libm's in
 * its last places.  No grain is written anywhere. */
#define FLANHIP_GRAIN_HANN 1
typedef struct flanhip_grain_event
	{
	uint64_t src;          /* the source's channel 0, frame 0: an offset in floats into `sources` where the call has one, else a device address */
	int64_t ch_stride;     /* floats between the source's channels */
	int64_t src_frames;    /* frames of a channel of the source: s + n <= src_frames */
	int64_t o;             /* the first output frame; may be negative */
	int64_t gain_offset;   /* >= 0: n per-frame gains from this offset of the gain pool; < 0: the scalar `gain` */
	int32_t s;             /* the first source frame */
	int32_t n;             /* frames; 0: an empty event (a null grain), which counts for the output's length alone */
	int32_t channels;      /* the source's channels; output channels from this on do not hear the event */
	int32_t sf, ef;        /* fade lengths in frames, sf + ef <= n */
	int32_t flags;         /* FLANHIP_GRAIN_HANN or 0 */
	float gain;
	int32_t reserved;
	} flanhip_grain_event;
/* the kernel's geometry: output frames per block, and events staged through LDS per round (what tests size their cases by) */
int64_t flanhip_grains_tile_frames(void);
int64_t flanhip_grains_batch_events(void);
/* integrate_event_rate (AudioSynthesis.cpp:310-374), host arithmetic: the event frames of length_frames frames.  rate / scatter: curves of
 * length_frames floats (the Functions sampled at f * ( 1.0f / sample_rate )) or, with NULL, the scalar; both clamped at 0 (:320, :323).
 * The fp32 accumulator starts at 1.0f, grows by rate / sample_rate per frame and drops its floor when it reaches 1 (:328-338): frame 0
 * always holds an event, and a rate of 0 yields that one alone.  Where scatter and rate are not 0 an event moves to
 * Frame( frame + sigma * z ), sigma = scatter / rate * sample_rate frames in fp32, z a normal deviate; events that land outside
 * [0, length_frames) are dropped and the rest sorted (:343-366).  The reference seeds std::default_random_engine from the clock; here
 * `seed` starts a splitmix64 stream read by Box and Muller's transform in double, so a seed names one result.  With scatter 0 nothing
 * is drawn and the result is exact.  Event i lies at time float( frame ) / sample_rate (:371).  out_frames: room for `capacity` frames
 * (length_frames always suffices); capacity 0 gives the count alone.  length_frames <= 0 and sample_rate <= 0 are refused. */
int flanhip_grains_events(int64_t length_frames, float sample_rate, const float * rate, float rate_scalar, const float * scatter, float scatter_scalar,
                          uint64_t seed, int64_t * out_frames, int64_t capacity, int64_t * out_count);
/* Audio::cut (AudioTemporal.cpp:190-205) for a table of grains of a source of num_frames frames, host arithmetic: fills s, n, sf, ef of
 * events[i] and nothing else.  Times become frames by time_to_frame truncated to Frame; granulate passes ( selection, selection + length,
 * fade, fade ) (AudioSynthesis.cpp:593).  Then flanhip_grains_cut_frames.  A time that is not finite or whose frame no Frame holds -- an
 * unvoiced psola grain is 2.0f / 0 long -- makes an EMPTY event, not an integer conversion of infinity. */
int flanhip_grains_cut(int64_t num_frames, float sample_rate, int64_t count, const float * start_time, const float * end_time,
                       const float * start_fade, const float * end_fade, flanhip_grain_event * events);
/* Audio::cut_frames (AudioTemporal.cpp:207-234): end <= start is an empty event, checked before the clamp (:217); start and end clamped to
 * [0, num_frames - 1] (:218-219), n = end - start; the fades clamped at 0 and, where sf + ef > n, both scaled by float( n ) / ( sf + ef )
 * and floored (AudioVolume.cpp:111-118). */
int flanhip_grains_cut_frames(int64_t num_frames, int64_t count, const int32_t * start, const int32_t * end, const int32_t * start_fade,
                              const int32_t * end_fade, flanhip_grain_event * events);
/* The output's length and the plan.  *out_frames on entry: 0 asks for the reference's length, max( o + n ) over ALL events from 0
 * (AudioCombination.cpp:146-150), which is written back; a positive value is the caller's own length (events are clipped to it, :162).
 * Unless both arrays are NULL, the plan for that length: per tile of flanhip_grains_tile_frames() output frames the first and the last
 * event index that touch it ( ( 0, -1 ): none ).  num_tiles must be ceil( length / tile ): ask for the length first.  Host arithmetic,
 * O( events + overlaps ). */
int flanhip_grains_plan(const flanhip_grain_event * events, int64_t count, int64_t * out_frames, int32_t * tile_first, int32_t * tile_last,
                        int64_t num_tiles);
/* bytes of device workspace flanhip_grains_mix_dev asks for: the table and the plan (0 for sizes it refuses) */
size_t flanhip_grains_workspace_bytes(int64_t count, int64_t out_frames);
/* The mix (AudioCombination.cpp:151-169), one launch.  events, tile_first, tile_last: HOST tables (they are checked here, then copied into
 * the workspace); d_gains: the pool of per-frame gains (NULL if no event has one); d_sources: where the events' src offsets start, or
 * NULL if they are device addresses; d_out: float[num_channels][out_frames], every element written.  Events may come in any order of o.
 * out_frames need not be the plan's maximum, but the plan must be made for it (num_tiles tiles).  Refused with FLANHIP_ERR_INVALID_ARG
 * before any device call: null pointers, non-positive sizes, sample_rate <= 0, an event whose source range leaves its buffer (s < 0,
 * s + n > src_frames, or its channels beyond sources_floats), whose fades exceed it, whose gains leave the pool, and a plan that names
 * events the table does not hold. */
int flanhip_grains_mix_dev(const flanhip_grain_event * events, int64_t count, const int32_t * tile_first, const int32_t * tile_last, int64_t num_tiles,
                           const float * d_gains, int64_t gain_floats, const float * d_sources, int64_t sources_floats, int64_t num_channels,
                           int64_t out_frames, float sample_rate, float * d_out, void * d_workspace, void * stream);
/* Host pointers; every src is an offset into `sources`; the plan is made here.  `cancel` is polled before the uploads, before the launch
 * and while it runs. */
int flanhip_grains_mix(const flanhip_grain_event * events, int64_t count, const float * gains, int64_t gain_floats, const float * sources,
                       int64_t sources_floats, int64_t num_channels, int64_t out_frames, float sample_rate, float * out, volatile int * cancel);

/* ---- Audio silence removal and slicing: get_loud_chunks, remove_silence, remove_edge_silence, reverse, the splits, rearrange, random_chunks
 * (Audio/AudioTemporal.cpp:10-188, 409-546) (flan_amd/csrc/temporal.hip) ------------------------------------------------ */
/* The loud chunks of get_loud_chunks_base (AudioTemporal.cpp:20-48).  Frame f is NOISY when sample( c, f ) > level for some channel c: a
 * signed compare (a loud negative sample is not noisy), false for a NaN.  A chunk starts at a noisy frame met in a quiet sector and is closed
 * by the first frame more than gap_frames after the last noisy one, with that last noisy frame as its end (:41-45); a chunk still open after
 * the last frame ends at num_frames (:47-48).  A negative gap makes every noisy frame a chunk { f, f }.  On the device the loop is a scan of
 * maps ( first, last, inner chunk starts ) over runs of frames: results do not depend on the run.
 * summary: int64[4] = { chunk count, first noisy frame, last noisy frame, 0 }, the frames -1 when nothing is noisy.
 * chunks: int32[count][2] = { start, end }.
 * flanhip_loud_summary_dev launches the detection and leaves the summary; flanhip_loud_chunks_dev, on the same workspace and with the same
 * num_channels, num_frames and gap_frames, writes the table: `count` is what the caller read from the summary and the kernel's own limit --
 * nothing is ever written at or past entry `count` --, and a capacity (the entries d_chunks has room for) below it is refused.  Refused with FLANHIP_ERR_INVALID_ARG before any device call: null pointers, sizes
 * <= 0, num_frames > INT32_MAX. */
size_t flanhip_loud_workspace_bytes(int64_t num_channels, int64_t num_frames);
int flanhip_loud_summary_dev(const float * d_audio, int64_t num_channels, int64_t num_frames, float level, int64_t gap_frames, int64_t * d_summary,
                             void * d_workspace, void * stream);
int flanhip_loud_chunks_dev(int64_t num_channels, int64_t num_frames, int64_t gap_frames, int64_t count, int32_t * d_chunks, int64_t capacity,
                            void * d_workspace, void * stream);
/* Host pointers, the whole call: the summary always; the table if capacity > 0, which must then hold the count (capacity 0 asks for the
 * summary alone).  `cancel` is polled before the uploads, before the launches and while they run. */
int flanhip_loud_chunks(const float * audio, int64_t num_channels, int64_t num_frames, float level, int64_t gap_frames, int32_t * chunks,
                        int64_t capacity, int64_t * summary, volatile int * cancel);
/* test hook: frames per lane of the detection's kernels for the calling thread (1 ... 64; 0: the library's choice), which also sizes the
 * workspace; and the geometry in force: frames per lane and per block, and the blocks the carry kernel takes per pass (what tests size
 * their cases by) */
void flanhip_loud_debug_run(int frames);
int64_t flanhip_loud_run_frames(void);
int64_t flanhip_loud_block_frames(void);
int64_t flanhip_loud_carry_pass_blocks(void);
/* Audio::reverse (AudioTemporal.cpp:174-188): out[c][f] = in[c][num_frames - 1 - f].  16-byte stores on the output's own boundaries whatever
 * num_frames and the rows' alignment are.  The two buffers must not overlap at all: an output that shares any byte with the input is
 * refused with FLANHIP_ERR_INVALID_ARG. */
int flanhip_audio_reverse_dev(const float * d_audio, int64_t num_channels, int64_t num_frames, float * d_out, void * stream);
int flanhip_audio_reverse(const float * audio, int64_t num_channels, int64_t num_frames, float * out, volatile int * cancel);
/* The fades and cuts of get_loud_chunks_base (AudioTemporal.cpp:52-83), host arithmetic, quirks kept: fade_ins has count + 1 entries, all
 * fade_in_time at first; iteration i reads fade_ins[i] AFTER iteration i - 1 overwrote it (:57 after :61), sets fade_ins[i] to the chunk's start
 * where the fade would reach before frame 0 and fade_ins[i + 1] to num_frames - end where it would reach num_frames, every value going through
 * frame_to_time and back through time_to_frame in fp32; chunk i is cut_frames( start - left, end + right, left, right ) by
 * flanhip_grains_cut_frames' rules -- whose clamp of the end to num_frames - 1 costs a chunk that reaches the end its last frame --, filling s,
 * n, sf, ef of events[i].  offsets (count + 1 floats, or NULL): -2 * fade_ins[i] (:82-83).  join != 0: also every event's o, by Audio::join's
 * fp32 running sum ( start + n / sample_rate ) + offsets[i + 1] (AudioCombination.cpp:205-221) and mix's time_to_frame (:127-129): the table of
 * remove_silence.  chunks: int32[count][2] inside [0, num_frames].  Refused: null pointers, sizes <= 0, num_frames > INT32_MAX,
 * sample_rate <= 0, a count flanhip_grains_workspace_bytes refuses, a fade no Frame holds. */
int flanhip_loud_chunks_fades(int64_t num_frames, float sample_rate, const int32_t * chunks, int64_t count, float fade_in_time, int join,
                              flanhip_grain_event * events, float * offsets);
/* remove_edge_silence's cut (AudioTemporal.cpp:149-152) from the summary's first and last noisy frame (both -1: nothing noisy, which the
 * reference's loops turn into start num_frames and end 0): out4 = { start - fade, end + fade, start fade, end fade } for cut_frames, with
 * start = first, end = last + 1 and the fades shortened where they would leave the signal. */
int flanhip_edge_silence_cut(int64_t num_frames, float sample_rate, int64_t first_noisy, int64_t last_noisy, float fade_time, int32_t * out4);
/* split_at_times' frames (AudioTemporal.cpp:416-429): 0, then the frames of the SORTED times, skipping frames <= 0 and stopping at the first
 * >= num_frames, then num_frames; piece i is cut_frames( frames[i], frames[i + 1], fade, fade ).  *out_count: the number of frames (pieces + 1);
 * capacity 0 gives the count alone (count + 2 always suffices).  A NaN time is refused. */
int flanhip_split_frames(int64_t num_frames, float sample_rate, const float * times, int64_t count, int32_t * frames, int64_t capacity,
                         int64_t * out_count);
/* rearrange's order (AudioTemporal.cpp:477-479).  The reference calls std::shuffle, whose draws the standard does not fix; here the permutation
 * is this Fisher-Yates: order = 0 ... count - 1, g = std::mt19937( uint32( seed ) ), and for i = count - 1 down to 1: swap( order[i],
 * order[g() % ( i + 1 )] ).  Output slot i plays slice order[i].  A seed names one result on every platform. */
int flanhip_rearrange_order(int64_t count, uint64_t seed, int32_t * order);
/* random_chunks' plan (AudioTemporal.cpp:493-533).  flanhip_random_chunks_frames: the iterations L of the loop at :496, which compares a Frame
 * with the float time_to_frame( length ) (so a fractional end counts one more frame); -1 for what it refuses.  chunk_length: L floats, the
 * Function at frame_to_time( f ), or NULL for the scalar; fade: L + 1 floats, or NULL.  The accumulator is a double and starts at 1; a chunk's
 * length is clamped to [ frame_to_time( 32 ), num_frames / sample_rate ] in fp32; the starts end with Frame( time_to_frame( length ) ).  Chunk i is
 * cut_frames( start, start + desired, left, right ) with desired = its frames + time_to_frame( ( fade_i + fade_i+1 ) / 2 ) and start = 0 where
 * desired >= num_frames, else std::mt19937( uint32( seed ) )() % ( num_frames - desired ), drawn in chunk order: portable, so a seed names one
 * result.  events: s, n, sf, ef and o (join with offsets[i] = -fade_i, as above); chunk_starts: the chunks' output frames (the mod's times);
 * offsets: count + 1 floats.  capacity 0 gives the count alone. */
int64_t flanhip_random_chunks_frames(float sample_rate, float length);
int flanhip_random_chunks_plan(int64_t num_frames, float sample_rate, float length, const float * chunk_length, float chunk_length_scalar,
                               const float * fade, float fade_scalar, uint64_t seed, flanhip_grain_event * events, int32_t * chunk_starts,
                               float * offsets, int64_t capacity, int64_t * out_count);

/* ---- Audio::resample (Audio/AudioConversions.cpp:14-30, r8brain CDSPResampler with default parameters) --------- */
/* AudioConversions.cpp:22: out frames = Frame( float(num_frames) * ( dst_rate / src_rate ) ) */
int64_t flanhip_resample_out_frames(int64_t num_frames, float src_rate, float dst_rate);
/* in: float[ch][n]; out: float[ch][flanhip_resample_out_frames(n,...)].  Like the reference, the whole channel-major buffer is
 * resampled as ONE stream (filter ringing crosses channel boundaries).  Every chain CDSPResampler builds for two positive rates is served
 * (r8brain/CDSPResampler.h:119-378): one block convolver (2:1 -- 96 -> 48 kHz, the tuned kernel --, 3:1, 3:2, 2:3, 4:3, 1:2, 1:3); block
 * convolver + half-band upsamplers (4x, 8x ..., 6x, 12x ...); 2x convolver + fractional interpolator (44.1 <-> 48 kHz ...: whole stepping, or the
 * spline-interpolated bank for rates without a small common divisor, e.g. 44.1 kHz -> 48001 Hz); intermediate interpolation (8 -> 44.1 kHz,
 * 44.1 -> 192 kHz: 2x convolver, interpolator, a 2x convolver whose transition band follows from the rates, half-band upsamplers); half-band
 * downsamplers + convolver [+ interpolator] (192 -> 48, 96 -> 16, 192 -> 44.1 kHz ...).  Chains of several stages take transient fp64 streams
 * from the stream's memory pool; a chain with the spline bank synchronises the stream once (a small table goes up) and, like the reference,
 * its result depends on num_frames (r8brain re-bases the interpolator's position counter once per process() call = per num_frames input
 * samples).  Results: bit-identical to the vendored r8brain on the committed vectors (tests/golden/ref_made/r8brain.npz) but for samples
 * within rounding of a tie (>= 99.9 % identical, the rest one fp32 ulp). */
int flanhip_resample(const float * in, int64_t num_channels, int64_t num_frames, float src_rate, float dst_rate,
                     float * out, volatile int * cancel);
int flanhip_resample_dev(const float * d_in, int64_t num_channels, int64_t num_frames, float src_rate, float dst_rate,
                         float * d_out, void * stream);

/* ---- a PV that is a FRAME RANGE of a longer one (few channels, long signals: frame ranges instead of channels shard across
 * GPUs).  Analysis needs nothing new (a range of frames depends only on the samples under its windows and on the
 * frame before it).  Synthesis integrates the phase over ALL earlier frames, so it runs in two steps with one small exchange
 * between them:  (1) every rank: flanhip_synthesize_prepass_dev -> d_total_out[ch][bins], the phase its own frames add up to
 * (mod pi2), the chain sums stay in the workspace;  (2) the ranks exchange the totals; rank r folds the totals of ranks < r into
 * d_carry_in and calls flanhip_synthesize_dev_carry.  Samples within window/2 of a range boundary receive contributions from
 * both neighbours: flan_amd/sharding.py pads each range with silent frames so that they land inside the local output, and adds
 * the overlaps.  NaN flag as in flanhip_synthesize_dev (step 1 scans the data). ------------------------------------------------- */
int flanhip_synthesize_prepass_dev(const flanhip_MF * d_pv, int64_t num_channels, int64_t num_pv_frames, int num_bins,
                                   float sample_rate, float analysis_rate, int window_size, void * d_workspace,
                                   double * d_total_out, int * d_nan_flag, void * stream);
int flanhip_synthesize_dev_carry(const flanhip_MF * d_pv, int64_t num_channels, int64_t num_pv_frames, int num_bins,
                                 float sample_rate, float analysis_rate, int window_size, float * d_out, void * d_workspace,
                                 const double * d_carry_in, int * d_nan_flag, void * stream);

/* ---- multi-GPU: reassembling the channel shards of the output.  One process per GPU; channels shard with no
 * exchange during compute; the output step is ONE in-place all-gather over RCCL / xGMI.  RCCL is bound at run time (dlopen):
 * without librccl.so these four return FLANHIP_ERR_UNSUPPORTED and everything else still works. ------------------------- */
#define FLANHIP_COMM_ID_BYTES 128                     /* ncclUniqueId */
/* rank 0 creates the id and hands the 128 bytes to the other ranks by whatever launcher it uses (MPI, a file, a socket ...) */
int flanhip_comm_unique_id(char * id_out /* [FLANHIP_COMM_ID_BYTES] */);
/* collective over all ranks; the device is the one current in this process (flanhip_set_device).  comm_out: an ncclComm_t */
int flanhip_comm_init(const char * id, int world_size, int rank, void ** comm_out);
int flanhip_comm_destroy(void * comm);
/* d_all: float[world_size][count_per_rank]; this rank's shard (its channels, Audio layout float[ch][frames]) is already at
 * d_all + rank * count_per_rank.  On return (stream order) d_all is the whole float[all channels][frames] buffer on every rank.
 * comm may also be an ncclComm_t created elsewhere with the same RCCL. */
int flanhip_allgather_audio(void * comm, float * d_all, int64_t count_per_rank, int rank, void * stream);

/* ---- flan::Wavetable (Wavetable.cpp; WDL/resample.cpp) (flan_amd/csrc/wavetable.hip) --------------------------------- */
/* A wavetable is float[ch][slots * W]: `slots` waveforms of W frames per channel.  slots = the largest number of waveform starts of any
 * channel (:77-79); a channel with k starts fills k - 1 slots and the rest stay 0, as in the reference, whose synthesize reads them. */
#define FLANHIP_WAVETABLE_SNAP_NONE 0
#define FLANHIP_WAVETABLE_SNAP_ZERO 1
#define FLANHIP_WAVETABLE_SNAP_LEVEL 2
#define FLANHIP_WAVETABLE_PITCH_NONE 0
#define FLANHIP_WAVETABLE_PITCH_LOCAL 1
#define FLANHIP_WAVETABLE_PITCH_GLOBAL 2
#define FLANHIP_WAVETABLE_NORMALIZE 0
#define FLANHIP_WAVETABLE_REMOVE_DC 1
#define FLANHIP_WAVETABLE_ADD_FADES 2
#define FLANHIP_WAVETABLE_REMOVE_JUMPS 3
/* snap_frame_to_sample (:19-60) on one channel row, host-only, restated literally: the two-sided search with its asymmetric limits
 * ( left >= max( frame - distance, 0 ), right < min( frame + distance, n - 1 ) ), left + 1 on a left hit, and the fallback to the frame
 * whose | data - height | * ( 1 + | f - frame | / distance ) is smallest.  A distance of 0 (or below) returns frame_to_snap, as the
 * reference's NaN comparisons do.  frame_to_snap outside [0, num_frames) is FLANHIP_ERR_INVALID_ARG. */
int flanhip_wavetable_snap(const float * row, int64_t num_frames, int32_t frame_to_snap, float snap_height, int32_t search_distance, int32_t * out);
/* get_waveform_starts' walk for ONE channel (:181-214), host-only.  row: the UNFILTERED source row (what the snapping reads);
 * local_wavelengths: get_local_wavelengths( c, 0, -1, W, 128, 1, 32 ) of the low-passed copy (read in Local mode only, truncated to a
 * Frame per entry, :193); global_wavelength: get_average_wavelength truncated to a Frame (-1 stays -1; 0 when the pitch mode is None,
 * :158); pitch_mode: the mode in force for this channel (the caller carries Global -> None over to later channels, :163-164);
 * max_snap = Frame( snap_ratio * expected ).  The checks of :145-146 (fixed_frame < 1, snap_ratio outside ( 0, .95 )) are
 * FLANHIP_ERR_INVALID_ARG here; the C++ constructor makes a null Wavetable of them.  out: room for `capacity` starts (capacity 0: the count
 * alone); *out_count: how many the walk made.  Deviation: an expected wavelength below 1 (a global wavelength of 0) or a walk that makes
 * more than 2 num_frames starts never ends in the reference; FLANHIP_ERR_UNSUPPORTED here. */
int flanhip_wavetable_starts(const float * row, int64_t num_frames, const float * local_wavelengths, int64_t num_locals, int32_t global_wavelength,
                             int snap_mode, int pitch_mode, float snap_ratio, int32_t fixed_frame, volatile int * cancel, int32_t * out,
                             int64_t capacity, int64_t * out_count);
/* ratio_to_table_index (:463-488) for one channel's starts, host-only, fp32 as written: source_frame = Frame( r * num_source_frames ),
 * the upper_bound, the clamps.  (A product no Frame holds saturates; NaN is 0.) */
int flanhip_wavetable_table_index(const int32_t * starts, int64_t count, int32_t num_source_frames, const float * ratio, int64_t num, float * out);
/* the slots of a table: max counts[c] (0 for null / empty arguments) */
int64_t flanhip_wavetable_slots(const int64_t * counts, int64_t num_channels);
/* resample_waveforms (:67-132).  starts: the channels' start lists one after another (HOST memory in every form), counts[c] of them for
 * channel c.  Waveform w of channel c is the n = starts[c][w+1] - starts[c][w] source frames from starts[c][w]; its slot receives
 *   y = c2r_W( zero-padded or truncated r2c_n( x ) )    both transforms unnormalised, c2r ignoring the imaginary parts of bins 0 and W/2
 *   zero_crossing_frame: offsets 1 ... Frame( W * 0.1f ), y[W - offset] before y[offset], the first whose ( y > 0 ) differs from y[0]'s; else 0
 *   table[c][w W + f] = y[( zero_crossing_frame + f ) % W] / sqrtf( float( n * n ) )
 * The forward transform is min( n/2, W/2 ) + 1 direct sums (n may be odd): fp32 products chained 32 at a time, the chunks added in fp64,
 * with twiddles rounded from fp64; the inverse is the project's fp32 FFT.  Not bit-identical to FFTW; DESIGN.md 4.23 gives the error.
 * rotations (nullable): int32[ch][slots], every waveform's zero_crossing_frame (0 for empty slots).  Every element of table is written.
 * W must be a power of two in 64 ... 8192 and n <= 16384 (the samples stay in LDS), else FLANHIP_ERR_UNSUPPORTED; a waveform that
 * leaves [0, num_frames) is FLANHIP_ERR_INVALID_ARG.  Deviations: where n/2 + 1 > W/2 + 1 the reference copies past the end of its
 * spectrum (:100), here W/2 + 1 bins are copied; n <= 0, for which the reference plans a transform of size 0, leaves the slot 0. */
size_t flanhip_wavetable_resample_workspace_bytes(int64_t num_channels, int64_t num_frames, const int32_t * starts, const int64_t * counts, int32_t wavelength);
int flanhip_wavetable_resample_dev(const float * d_audio, int64_t num_channels, int64_t num_frames, const int32_t * starts, const int64_t * counts,
                                   int32_t wavelength, float * d_table, int32_t * d_rotations, void * d_workspace, void * stream);
int flanhip_wavetable_resample(const float * audio, int64_t num_channels, int64_t num_frames, const int32_t * starts, const int64_t * counts,
                               int32_t wavelength, float * table, int32_t * rotations, volatile int * cancel);
/* Wavetable::synthesize's resampler state (:293-330 over ResamplePrepare :1218-1265 and ResampleOut :1313-1343, :1558-1566 of
 * WDL/resample.cpp, SetMode( true, 1, true ): the 64-tap sinc, not feeding), host-only, in fp64 with the reference's own chain of
 * srcpos += ratio.  Per block: rate_in = max( freq, 1 ), rate_out = max( sample_rate / W, 1 ) (the argument order of :307),
 * wanted = int( ratio g ) + 4 + 64 - S after the prelude of 31 zeros of the first call.  ResampleOut is asked for ALL remaining frames, so
 * a block delivers until its input ends (ipos >= filtlen - 1, :1343) -- about g + 3 / ratio frames, not g -- and the next block starts
 * there: first_out[b + 1] = first_out[b] + num_out[b], and the loop ends exactly at out_frames.  freq: the frequency Function sampled at
 * every output frame (freq[min( frame, freq_count - 1 )]; one entry for a constant); a block reads the entry of its first frame (:300).
 * in_start[b]: input samples appended before block b, so that its phase_frame (:329) is in_start[b] % W.  Returns the number of blocks
 * (the arrays, each nullable, are filled up to `capacity`) or a negative error: g < 1 (the reference would not end) and a frequency that
 * is not finite are FLANHIP_ERR_INVALID_ARG; a ratio above 34 after the first block, where the reference's buffer drops below its
 * prelude and it reads samples it no longer holds, is FLANHIP_ERR_UNSUPPORTED. */
int64_t flanhip_wavetable_synth_plan(int64_t out_frames, float sample_rate, int32_t wavelength, int64_t granularity_frames, const float * freq,
                                     int64_t freq_count, int64_t capacity, int64_t * offsets, double * fracpos, double * ratio, double * filtpos,
                                     int32_t * oversize, int32_t * ideal, int64_t * first_out, int32_t * num_out, int32_t * wanted, int64_t * in_start);
/* How the synthesis launch cuts that plan into runs (host arithmetic, no device; the launch's own planner, for tests that must know which
 * path a shape takes): a run is consecutive output frames that one workgroup computes from one coefficient table and one staged stream
 * window.  Returns the number of runs or a negative FLANHIP_ERR_* as the plan does (num_channels <= 0: FLANHIP_ERR_INVALID_ARG), and fills the
 * first `capacity` records of every array that is not null: the run's first output frame and frame count, the block of its first frame
 * and how many blocks its frames lie in, j0 (the run's first frame is output j0 of that block: above 0 only where a block was cut into
 * pieces), and the staged window [win_start, win_start + win_len), which holds every tap of the run.  *channels_per_group / *groups
 * (nullable): the channels one workgroup walks and the groups per run for num_channels channels (the grid is runs x groups). */
int64_t flanhip_wavetable_synth_runs(int64_t out_frames, float sample_rate, int32_t wavelength, int64_t granularity_frames, const float * freq,
                                     int64_t freq_count, int64_t num_channels, int64_t capacity, int64_t * first_out, int32_t * num_out,
                                     int64_t * first_block, int32_t * num_blocks, int64_t * j0, int64_t * win_start, int32_t * win_len,
                                     int32_t * channels_per_group, int64_t * groups);
/* Wavetable::synthesize (:266-334).  table: float[ch][slots W]; freq: as above (HOST); index: float[ch][num_blocks] (HOST), the table
 * index of every ( channel, block ) -- ratio_to_table_index of the ratio Function at the block's first frame, within [0, slots - 1] --;
 * out: float[ch][out_frames], every element written.  Input sample t, appended by the block q with in_start[q] <= t < in_start[q] + wanted[q], is
 *   ( 1.0f - rem ) * table[c][t % W + W left] + rem * table[c][t % W + W right]     left = floor( index ), right = ceil( index ), rem = index - left
 * every operation rounded (:316-318), or the left term alone without `smooth` (:322-323); the output samples are the resampler's tap sums
 * (flanhip_audio_repitch's, wdl_sinc.h) at the positions of the reference's own chain of srcpos += ratio, which one lane per block walks
 * before the sums: what is left to differ from the reference is the rounding of a table coefficient.  num_blocks must be the plan's. */
size_t flanhip_wavetable_synth_workspace_bytes(int64_t num_channels, int64_t out_frames, float sample_rate, int32_t wavelength,
                                               int64_t granularity_frames, const float * freq, int64_t freq_count);
int flanhip_wavetable_synth_dev(const float * d_table, int64_t num_channels, int64_t slots, int32_t wavelength, float sample_rate, int64_t out_frames,
                                int64_t granularity_frames, const float * freq, int64_t freq_count, const float * index, int64_t num_blocks, int smooth,
                                float * d_out, void * d_workspace, void * stream);
int flanhip_wavetable_synth(const float * table, int64_t num_channels, int64_t slots, int32_t wavelength, float sample_rate, int64_t out_frames,
                            int64_t granularity_frames, const float * freq, int64_t freq_count, const float * index, int64_t num_blocks, int smooth,
                            float * out, volatile int * cancel);
/* normalize_in_place (:429-451: the slot's exact max |s|, untouched below 0.001, else s / max), remove_dc_in_place (:414-427: s - sum / W,
 * the fp32 sum in a fixed tree order, not the reference's left-to-right one), add_fades_in_place (:364-384) and remove_jumps_in_place
 * (:386-412): fade = sinf( pi / 2.0f * ( frame + 1 ) / fade_frames ) for frame < fade_frames - 1 on wf[frame] and wf[W - 1 - frame], in
 * the order of the frames where the two edges overlap.  In place, every slot of every channel once.  Deviations: the reference's fade
 * loops nest a second channel loop in a parallel one and edit a slot once per channel from racing threads; frames past the waveform
 * (fade_frames - 1 > W), which the reference writes out of bounds, are left out. */
int flanhip_wavetable_edit_dev(float * d_table, int64_t num_channels, int64_t slots, int32_t wavelength, int mode, int32_t fade_frames, void * stream);
int flanhip_wavetable_edit(float * table, int64_t num_channels, int64_t slots, int32_t wavelength, int mode, int32_t fade_frames, volatile int * cancel);

/* ---- Audio::synthesize_spectrum (Audio/AudioSynthesis.cpp:151-268; WDL/resample.cpp) (flan_amd/csrc/spectrum.hip) ------ */
/* N = 2^spectrum_size_power table frames, C = N/2, B = C + 1 bins, fundamental = 2^fundamental_power, the table's sample rate 48000.
 * Host-only helpers (no device needed), the reference's fp32 arithmetic:
 *   bins           freq[b] = b * 48000 / float( B ) (:186 -- by B, not N) and harmonic[b] = int( round( freq[b] / fundamental ) ) (:201), each array
 *                  nullable and filled up to `capacity`; returns B (0 for powers outside 1 ... 30 / 0 ... 30)
 *   num_harmonics  ceil( 48000 / fundamental ) + 1 (:188): spread and harmonic_scale are sampled at harmonics 1 ... num_harmonics (:190-196)
 *   phases         std::mt19937( seed ) and one std::uniform_real_distribution<float>( 0, 2 pi ) draw (:212) per bin with harmonic != 0 in ascending
 *                  bin order, 0 elsewhere (the reference seeds from std::random_device and draws in the order its parallel loop reaches the bins)
 *   jump           Frame( ( float( channel ) / num_channels ) * N ) (:236), channel c's phase offset into the table */
int64_t flanhip_spectrum_bins(int32_t spectrum_size_power, int32_t fundamental_power, int32_t * harmonic, float * freq, int64_t capacity);
int32_t flanhip_spectrum_num_harmonics(int32_t fundamental_power);
int flanhip_spectrum_phases(uint32_t seed, const int32_t * harmonic, int64_t bins, float * theta);
int32_t flanhip_spectrum_jump(int64_t channel, int64_t num_channels, int32_t spectrum_size_power);
/* The table (:198-219): bin b holds polar( mag[b], theta[b] ) (:214), formed in fp32, and fftwf_plan_dft_c2r_1d( N ) -- unnormalised, the
 * imaginary parts of bins 0 and C ignored -- gives
 *   table[n] = Re X0 + (-1)^n Re X_C + 2 sum_{k=1}^{C-1} Re( X_k exp( +2 pi i k n / N ) ).
 * mag, theta: float[B]; table: float[N].  Bins the reference skips ( harmonic == 0, :202 ) it leaves as whatever fftwf_alloc_complex
 * returned; here they are what the caller passes, and the callers of this library pass ZERO.  6 <= spectrum_size_power <= 22, else
 * FLANHIP_ERR_UNSUPPORTED (the reference accepts up to 31).  Up to 13 one workgroup transforms the C complex points in LDS; above, C = C1 C2
 * in two passes through the workspace ( C1 = max( 16, C / 4096 ) ), twiddles from sincospi of exact dyadic arguments.  Fixed summation
 * order: two runs agree bit for bit.  Workspace: 8 C bytes. */
size_t flanhip_spectrum_table_workspace_bytes(int32_t spectrum_size_power);   /* 0 for arguments it refuses */
int flanhip_spectrum_table_dev(const float * d_mag, const float * d_theta, int32_t spectrum_size_power, float * d_table, void * d_workspace,
                               void * stream);
int flanhip_spectrum_table(const float * mag, const float * theta, int32_t spectrum_size_power, float * table, volatile int * cancel);
/* The loop (:230-263): flanhip_wavetable_synth's resampler over ONE row of W = 2^table_size_power frames, one slot, no blend, with
 * SetRates( max( freq, 1 ), max( rate_out, 1 ) ) (:247; rate_out = the fundamental) and input sample t of channel c read at
 * table[( t + jump_c ) % W], jump_c = flanhip_spectrum_jump( c, num_channels, table_size_power ) computed inside (:254).  freq: HOST, per
 * output frame or one entry, as flanhip_wavetable_synth takes it; out: float[ch][out_frames].  The block plan does not depend on the channel;
 * flanhip_spectrum_synth_plan returns it as flanhip_wavetable_synth_plan does, with the same refusals (a ratio above 34 after the first
 * block, a granularity below one frame, a frequency that is not finite). */
int64_t flanhip_spectrum_synth_plan(int64_t out_frames, double rate_out, int64_t granularity_frames, const float * freq, int64_t freq_count,
                                    int64_t capacity, int64_t * offsets, double * fracpos, double * ratio, double * filtpos, int32_t * oversize,
                                    int32_t * ideal, int64_t * first_out, int32_t * num_out, int32_t * wanted, int64_t * in_start);
size_t flanhip_spectrum_synth_workspace_bytes(int32_t table_size_power, double rate_out, int64_t num_channels, int64_t out_frames,
                                              int64_t granularity_frames, const float * freq, int64_t freq_count);   /* 0 for arguments it refuses */
int flanhip_spectrum_synth_dev(const float * d_table, int32_t table_size_power, double rate_out, int64_t num_channels, int64_t out_frames,
                               int64_t granularity_frames, const float * freq, int64_t freq_count, float * d_out, void * d_workspace, void * stream);
int flanhip_spectrum_synth(const float * table, int32_t table_size_power, double rate_out, int64_t num_channels, int64_t out_frames,
                           int64_t granularity_frames, const float * freq, int64_t freq_count, float * out, volatile int * cancel);
/* Audio::synthesize_spectrum after its Functions have been sampled (:198-265), without leaving the device: flanhip_spectrum_table into the
 * workspace, flanhip_spectrum_synth with rate_out = 2^fundamental_power, then flanhip_audio_set_volume_dev at 48000 with level 1 (:265; it
 * does not look at the last frame).  out_frames = Frame( length * 48000.0f ), granularity_frames = Frame( granularity_time * 48000.0f )
 * (:225-228).  fundamental_power outside 1 ... spectrum_size_power is FLANHIP_ERR_INVALID_ARG (:164-166). */
size_t flanhip_audio_synthesize_spectrum_workspace_bytes(int32_t spectrum_size_power, int32_t fundamental_power, int64_t num_channels,
                                                         int64_t out_frames, int64_t granularity_frames, const float * freq, int64_t freq_count);
int flanhip_audio_synthesize_spectrum_dev(const float * d_mag, const float * d_theta, int32_t spectrum_size_power, int32_t fundamental_power,
                                          int64_t num_channels, int64_t out_frames, int64_t granularity_frames, const float * freq,
                                          int64_t freq_count, float * d_out, void * d_workspace, void * stream);
int flanhip_audio_synthesize_spectrum(const float * mag, const float * theta, int32_t spectrum_size_power, int32_t fundamental_power,
                                      int64_t num_channels, int64_t out_frames, int64_t granularity_frames, const float * freq, int64_t freq_count,
                                      float * out, volatile int * cancel);

/* ---- Audio::ring_modulate, the fades, add_moisture's nonlinearity, the named waveforms and get_total_energy (Audio/AudioVolume.cpp:15-30,
 * 69-188, Function.cpp:32-39, Audio/AudioInformation.cpp:121-129) (flan_amd/csrc/volume.hip) ---------------------------- */
/* The pointwise entry points below store 16 bytes per lane on the output's own 16-byte boundaries whatever num_frames and the rows' alignment
 * are.  d_out may be the input block itself; an output that shares bytes with an input without being it, or with a table, is refused.
 * Refused with FLANHIP_ERR_INVALID_ARG before any device call: null pointers, sizes <= 0, num_frames > INT32_MAX. */
/* Audio::ring_modulate (AudioVolume.cpp:15-30): out[c][f] = audio[c][f] * other[c % other_channels][f % other_frames], one fp32 product. */
int flanhip_audio_ring_modulate_dev(const float * d_audio, int64_t num_channels, int64_t num_frames, const float * d_other, int64_t other_channels,
                                    int64_t other_frames, float * d_out, void * stream);
/* fade_frames_in_place's validation (:111-118), host arithmetic: negative lengths become 0; where start + end > num_frames both are scaled by
 * float( num_frames ) / ( start + end ) in fp32 and floored.  out2 = { start, end }.  (The sum is formed in 64 bits; each result is kept at
 * num_frames at most.) */
int flanhip_fade_frames_plan(int64_t num_frames, int32_t start, int32_t end, int32_t * out2);
/* The two loops of fade_frames_in_place (:121-133) for every channel: frame f < start times d_start_gain[f], then frame num_frames - 1 - k,
 * k < end, times d_end_gain[k]; a frame in both ranges is multiplied twice, the start's gain first; every other frame is copied.  The tables
 * are what the host evaluated: interp( float( f ) / start ) and interp( float( k ) / end ).  A table may be NULL where its length is 0. */
int flanhip_audio_fade_dev(const float * d_audio, int64_t num_channels, int64_t num_frames, const float * d_start_gain, int64_t start,
                           const float * d_end_gain, int64_t end, float * d_out, void * stream);
/* The named waveforms (Function.cpp:32-39): t0 = fmod( t, 1.0f ) (which keeps t's sign), then sine sin( pi2 * t0 ), square t0 < 0.5f ? -1 : 1,
 * saw -1 + 2 t0, triangle t0 < 0.5f ? -1 + 4 t0 : 3 - 4 t0.  On the device the sine is the fp32 product pi2 * t0 and then the correctly
 * rounded fp32 sine (evaluated in fp64, rounded once); the other three are exact in fp32.  flanhip_waveform_host: the same on the host with
 * the C library's sinf. */
#define FLANHIP_WAVEFORM_SINE     0
#define FLANHIP_WAVEFORM_SQUARE   1
#define FLANHIP_WAVEFORM_SAW      2
#define FLANHIP_WAVEFORM_TRIANGLE 3
int flanhip_waveform_dev(int waveform_kind, const float * d_t, int64_t count, float * d_out, void * stream);
int flanhip_waveform_host(int waveform_kind, const float * t, int64_t count, float * out);
/* The shaper of Audio::add_moisture (:179-187) over the OVERSAMPLED block float[ch][oversampled_frames] at oversampled_rate, between the two
 * chains of Audio::waveshape (:153, :165).  Per sample s at oversampled frame F: t = float( F ) / oversampled_rate (:161); the curves are read
 * at i = Frame( t * sample_rate ), the ORIGINAL Audio's time_to_frame (:181-183), clamped to num_frames - 1 -- a stated deviation: for long
 * inputs the reference's fp32 arithmetic reaches num_frames and reads past its vector --; power = s >= 0 ? pow( s, skew ) : -pow( -s, skew );
 * out = s + amount * s * waveform( pi2 * frequency * power ), every product an fp32 product in that order, none contracted.  pow is
 * evaluated in fp64 and rounded once.  d_amount, d_frequency, d_skew: float[num_frames], or NULL for the scalar beside it. */
int flanhip_audio_moisture_dev(const float * d_oversampled, int64_t num_channels, int64_t oversampled_frames, float oversampled_rate,
                               int64_t num_frames, float sample_rate, const float * d_amount, float amount, const float * d_frequency,
                               float frequency, const float * d_skew, float skew, int waveform_kind, float * d_out, void * stream);
/* Audio::get_total_energy (AudioInformation.cpp:121-129): d_energy[c] = the sum of the channel's squares.  The squares are exact in fp64 and
 * are summed in fp64 in a fixed order (lane, wavefront, block, then the blocks by a second one-block launch), no atomics: two runs give the
 * same bits.  The sum is rounded to fp32 once: the result is the correctly rounded sum to within one ulp, NOT the rounding sequence of the
 * reference's sequential fp32 x + s * s (which its compiler may contract); a sum beyond fp32's range is inf. */
size_t flanhip_audio_energy_workspace_bytes(int64_t num_channels, int64_t num_frames);      /* 0 for a shape it refuses */
int flanhip_audio_energy_dev(const float * d_audio, int64_t num_channels, int64_t num_frames, float * d_energy, void * d_workspace, void * stream);
/* The rectifier of Audio::get_amplitude_envelope (AudioInformation.cpp:331-333): s < 0 ? s * -1 : s; -0 and a NaN stay as they are. */
int flanhip_audio_rectify_dev(const float * d_audio, int64_t num_channels, int64_t num_frames, float * d_out, void * stream);

/* ---- Audio::synthesize_waveform and synthesize_white_noise (Audio/AudioSynthesis.cpp:25-89) (volume.hip) ------------- */
/* Validation and sizes (:33-46): the output's frames Frame( length * sample_rate ), and through the pointers (either may be NULL) the input's
 * frames, that times oversample, and its rate, the fp32 product sample_rate * oversample as a double.  -1 for oversample < 1, length <= 0,
 * sample_rate <= 0, no output frame, or more input frames than a Frame counts. */
int64_t flanhip_synthesize_waveform_frames(float length, float sample_rate, int oversample, int64_t * num_in_frames, double * in_sample_rate);
/* The phases (:51-58): phase[i] = ( the sum of frequency[j], j < i, modulo M ) / M, M = in_sample_rate, a negative sum wrapping upward as
 * fmod_fixed does.  The reference forms them by std::exclusive_scan of fmod_fixed( a + b, M ) in fp32 under a parallel policy, whose grouping
 * is not defined; here the scan is carried in fp64 (a lane's run is one "add c modulo M" map, the maps are composed over the block and the
 * blocks), and phase = float( p / M ), one rounding: within 2^-23 of a cycle of the exact modular sum, which the reference's fp32 sums are not.
 * d_freq: float[num_in_frames] (the frequency Function sampled at i * ( 1.0f / M ), :46) or NULL for the scalar.  d_phases and d_wave:
 * float[num_in_frames]; either may be NULL; d_wave takes waveform( phase ) of the named kind.  The run -- frames per lane -- changes results
 * by fp64 rounding of the sums only. */
size_t flanhip_osc_workspace_bytes(int64_t num_in_frames);
int flanhip_osc_phase_dev(const float * d_freq, float freq, int64_t num_in_frames, double in_sample_rate, float * d_phases, float * d_wave,
                          int waveform_kind, void * d_workspace, void * stream);
/* test hook: frames per lane of the oscillator's scan for the calling thread (1 ... 64; 0: the library's choice), which also sizes the
 * workspace; and the geometry in force */
void flanhip_osc_debug_run(int frames);
int64_t flanhip_osc_run_frames(void);
int64_t flanhip_osc_block_frames(void);
int64_t flanhip_osc_carry_pass_blocks(void);
/* r8b::CDSPResampler( src_rate, dst_rate, num_in_frames ).oneshot( in, num_in_frames, out, num_out_frames ) (:65-66): the chain of
 * flanhip_resample_dev with the CALLER's output length.  Equal rates have no chain: the samples pass through (CDSPResampler.h:133-136),
 * zeros behind the input's end. */
int flanhip_oneshot_resample_dev(const float * d_in, int64_t num_in_frames, double src_rate, double dst_rate, float * d_out,
                                 int64_t num_out_frames, void * stream);
/* Audio::synthesize_waveform with a named waveform, without leaving the device: the scan with the waveform fused into its replay, then
 * flanhip_oneshot_resample_dev into exactly Frame( length * sample_rate ) frames.  d_freq as flanhip_osc_phase_dev takes it. */
size_t flanhip_audio_synthesize_waveform_workspace_bytes(float length, float sample_rate, int oversample);      /* 0 for arguments it refuses */
int flanhip_audio_synthesize_waveform_dev(int waveform_kind, const float * d_freq, float freq, float length, float sample_rate, int oversample,
                                          float * d_out, void * d_workspace, void * stream);
/* synthesize_white_noise's draw (:80-86), host: std::mt19937( seed ) through std::uniform_real_distribution<>( -1.0f, 1.0f ), each value
 * narrowed to fp32.  (The distribution is the C++ library's: two engine outputs per value in libstdc++.) */
int flanhip_white_noise_draw(uint64_t seed, int64_t count, float * out);

/* ---- synthetic input + comparison utilities (bench / tests; defined by this project) -------------- */
int flanhip_noise_dev(float * d_out, int64_t num_channels, int64_t num_audio_frames, uint32_t seed, void * stream);
/* a plain streaming copy, 16 bytes per lane: the measured-copy yardstick bench.py quotes beside the 8 TB/s spec (count: floats, a multiple of 4) */
int flanhip_copy_dev(const float * d_src, float * d_dst, int64_t count, void * stream);
/* sum of squares of (a - b) and of b, as doubles: d_result[0] = sum (a-b)^2, d_result[1] = sum b^2 */
int flanhip_sqdiff_dev(const float * d_a, const float * d_b, int64_t count, double * d_result, void * stream);

#ifdef __cplusplus
}
#endif
#endif /* FLANHIP_H */
