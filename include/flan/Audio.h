// flan/Audio.h -- the Audio side of the phase-vocoder path (mirrors the reference's src/flan/Audio/Audio.h:25-176 for
// construction and conversions; every method is const and returns a fresh object, invalid input gives a null object).
#pragma once
#include <complex>
#include <cstdint>
#include <limits>
#include <type_traits>
#include <utility>
#include <vector>

#include "flan/AudioBuffer.h"
#include "flan/AudioMod.h"
#include "flan/Function.h"
#include "flan/defines.h"
#include "flan/vec2.h"

namespace flan {

class PV;
class SPV;

/** The modes of WDL_Resampler that Audio::repitch offers (Audio/Audio.h:439-455, AudioTemporal.cpp:258-261). */
enum class WDLResampleType { Sinc, Linear, Uninterpolated };

class Audio : public AudioBuffer
	{
public:
	Audio();                                                                     // null Audio
	Audio( AudioBuffer && other );
	Audio copy() const;

	static Audio create_null();                                                  // prints "Null Audio created" (AudioConstructors.cpp:19-23)
	static Audio create_from_buffer( std::vector<float> && buffer, Channel num_channels, FrameRate sample_rate );   // Audio.h:62-66
	static Audio create_from_format( const AudioBuffer::Format & );
	static Audio create_empty_with_length( Second length, Channel num_channels = 1, FrameRate sample_rate = 48000.0f );
	static Audio create_empty_with_frames( Frame num_frames, Channel num_channels = 1, FrameRate sample_rate = 48000.0f ); // Audio.h:93-97

	// ---- conversions ----
	/** Windowed STFT + per-bin phase vocoding (Conversions/AudioPV.cpp:12-78).  dft_size: any EVEN size >= window_size up to 2^20 (the reference hands it
	 *  to FFTW as it is, FFTHelper.cpp:16-26).  Powers of two from 32 to 16384 run register / LDS FFT kernels (tuned ones at 256 ... 16384); sizes whose
	 *  half factors into 2 ... 13 a mixed-radix transform; sizes above 16384 whose half is C1 <= 256 times a product of 2 ... 13 up to 4096 (32768, 20000,
	 *  44100, 48000 ...) a two-level split; every other size up to 262144 (a large prime factor in the half) Bluestein's chirp-z form; only above that
	 *  what none of these serves falls to the direct sums (O( window x bins ) per frame, same results).
	 *  An odd size, or one below the window, returns a null PV. */
	PV convert_to_PV( Frame window_size = 2048, Frame hop = 128, Frame dft_size = 4096, flan_CANCEL_ARG ) const;  // Audio.h:158-163
	/** Stereo only: mid/side first (AudioPV.cpp:80-84). */
	PV convert_to_ms_PV( Frame window_size = 2048, Frame hop = 128, Frame dft_size = 4096, flan_CANCEL_ARG ) const;
	Audio convert_to_mid_side() const;                                           // AudioConversions.cpp:32-51
	Audio convert_to_left_right() const;                                         // :53-56
	/** The sliding-DFT vocoder (Conversions/AudioSPV.cpp:27-102): one spectrum of dft_size bins per input sample, on the device
	 *  (flanhip_spv_analyze_dev).  dft_size < 2 returns a null SPV (the reference reads bin 1 of every frame). */
	SPV convert_to_SPV( Bin dft_size = 1024, flan_CANCEL_ARG ) const;
	/** AudioSPV.cpp:104-108: convert_to_mid_side().convert_to_SPV( dft_size ) */
	SPV convert_to_ms_SPV( Bin dft_size = 1024, flan_CANCEL_ARG ) const;
	/** r8brain-equivalent sample-rate conversion (AudioConversions.cpp:14-30). */
	Audio resample( FrameRate new_sample_rate ) const;
	/** Convolution with an impulse response (Audio/AudioCombination.cpp:299-352), on the device (flanhip_convolve_dev).
	 *  A null *this or ir gives a null Audio; an ir of another sample rate is first ir.resample( get_sample_rate() ).  The result has
	 *  this Audio's channels and sample rate and n + m frames; IR channels are used cyclically (channel c takes ir channel c % ir channels).
	 *  normalize: the result times 1.0f / get_max_sample_magnitude(), so an all-zero result becomes NaN everywhere (0 * inf), as in the
	 *  reference.  The result stays device-resident until read. */
	Audio convolve( const Audio & ir, bool normalize = true ) const;
	/** Pitch and speed changed together by resampling at a rate that changes every `granularity` seconds (Audio/AudioTemporal.cpp:236-299,
	 *  over WDL_Resampler), on the device (flanhip_audio_repitch_dev).  factor is sampled once per granularity (at least one
	 *  frame) with Function::sample, each value becomes clamp( 1.0f / v, 1.0f / 1000, 1000 ); a constant behaves like the callable that returns
	 *  it.  Sinc: 64-tap windowed sinc; Uninterpolated: the nearest earlier sample; Linear is not built: a null Audio and one line on std::cout.
	 *  A null *this gives a null Audio.  The result stays device-resident until read. */
	Audio repitch( const Function<Second, float> & factor, Second granularity = .001f, WDLResampleType quality = WDLResampleType::Sinc ) const;

	// ---- volume ----
	/** Every sample times gain( t ), the same curve for every channel (Audio/AudioVolume.cpp:5-13, 32-44), on the device
	 *  (flanhip_audio_gain_dev).  gain is sampled once per frame at f * ( 1.0f / sample rate ); a constant is passed as it is
	 *  and samples nothing.  A null *this gives a null Audio (the in-place form leaves it as it is).  The result stays device-resident. */
	Audio modify_volume( const Function<Second, float> & gain ) const;
	Audio & modify_volume_in_place( const Function<Second, float> & gain );
	/** Normalise, then scale by level( t ) (:46-67): every sample times level / get_max_sample_magnitude(), one fp32 division and one fp32
	 *  product, on the device (flanhip_audio_set_volume_dev: the maximum never comes to the host).  As in the reference the maximum does not
	 *  look at the last frame (AudioBuffer.cpp:416-430), and a maximum of 0 returns the input unchanged. */
	Audio set_volume( const Function<Second, Amplitude> & level ) const;
	Audio & set_volume_in_place( const Function<Second, Amplitude> & level );
	/** The dynamic range compressor of :190-278 (Giannoulis, Massberg and Reiss, JAES 2012: gain computer with a soft knee, smooth decoupled
	 *  peak detector), on the device as two scans (flanhip_compress_dev).  Every parameter is sampled once per frame; a
	 *  constant samples nothing.  The detector reads the SIGNED maximum over the sidechain's channels, from 0 (:211-215 take no abs): frames
	 *  whose samples are all negative detect silence.  sidechain_source: null for *this.  Where the reference reads out of bounds -- a
	 *  sidechain with fewer frames than *this -- and for a null sidechain object the result is a null Audio; a longer sidechain is read up to
	 *  this Audio's length and its sample rate is not looked at.  The result stays device-resident until read. */
	Audio compress( const Function<Second, Decibel> & threshold, const Function<Second, float> & compression_ratio = 3.0f,
		const Function<Second, Second> & attack = 5.0f / 1000.0f, const Function<Second, Second> & release = 100.0f / 1000.0f,
		const Function<Second, Decibel> & knee_width = Decibel( 0 ), const Audio * sidechain_source = nullptr ) const;
	/** Every sample times the modulator's, whose channels and frames both wrap: out[c][f] = in[c][f] * other[c % channels][f % frames]
	 *  (Audio/AudioVolume.cpp:15-30), on the device (flanhip_audio_ring_modulate_dev), exact.  The modulator's sample rate is not
	 *  looked at.  A null *this or other gives a null Audio. */
	Audio ring_modulate( const Audio & other ) const;
	/** Fades over the first `start` and the last `end` frames (:69-135): frame f < start times interp( float( f ) / start ), frame frames - 1 - k,
	 *  k < end, times interp( float( k ) / end ).  Negative lengths are 0; lengths that together exceed the frames are both scaled by
	 *  float( frames ) / ( start + end ) and floored (flanhip_fade_frames_plan); a frame both fades reach is multiplied twice, the start's gain
	 *  first.  The interpolator, named or callable, is evaluated on the host into two small tables, so every one is exact; the frames are
	 *  multiplied on the device (flanhip_audio_fade_dev).  fade / fade_in_place: the times through time_to_frame, truncated.  Both fades 0
	 *  return a copy.  A null *this gives a null Audio; the in-place forms print "Null input" and leave it. */
	Audio fade( Second start = 16.0f / 48000.0f, Second end = 16.0f / 48000.0f, const Interpolator & interp = Interpolator::sqrt() ) const;
	Audio & fade_in_place( Second start = 16.0f / 48000.0f, Second end = 16.0f / 48000.0f, const Interpolator & interp = Interpolator::sqrt() );
	Audio fade_frames( Frame start = 16, Frame end = 16, const Interpolator & interp = Interpolator::sqrt() ) const;
	Audio & fade_frames_in_place( Frame start = 16, Frame end = 16, const Interpolator & interp = Interpolator::sqrt() );
	/** Every sample negated (:137-144): flanhip_audio_gain_dev with -1, an exact fp32 product. */
	Audio invert_phase() const;
	/** shaper( ( time, sample ) ) over every sample at oversample_factor times the sample rate (:146-166): resample( sr * k ) on the device,
	 *  ONE download, the shaper on the host over every ( channel, frame ) with ( oversampled.frame_to_time( frame ), s ) under the shaper's
	 *  policy, an upload, resample( sr ) on the device.  Equal bit for bit to that composition of the public methods.  A null *this, and
	 *  oversample_factor 0 (a sample rate of 0), give a null Audio. */
	Audio waveshape( const Function<std::pair<Second, Sample>, Sample> & shaper, uint16_t oversample_factor = 4 ) const;
	/** The moisture effect (:168-188): waveshape, factor 4, with s -> s + amount * s * waveform( pi2 * frequency * power ), power = s >= 0 ?
	 *  pow( s, skew ) : -pow( -s, skew ), the three Functions sampled once per ORIGINAL frame and read at Frame( time * sample rate ).  With a named
	 *  waveform (waveforms::sine, the default, square, saw, triangle) nothing leaves the device: the up-chain, flanhip_audio_moisture_dev, the
	 *  down-chain; a constant travels as a scalar.  Any other waveform takes waveshape with the reference's shaper on the host.  Stated
	 *  deviation: the curve index is clamped to frames - 1, where the reference's fp32 arithmetic can reach `frames` and read past its vector.
	 *  pow and sin are the correctly rounded fp32 functions on the device, the C library's on the host.  A null *this gives a null Audio. */
	Audio add_moisture( const Function<Second, Amplitude> & amount = .5f, const Function<Second, Frequency> & frequency = 96,
		const Function<Second, float> & skew = 4, const Waveform & waveform = waveforms::sine ) const;
	/** modify_volume( ADSR( ... ) ) (:280-301), and the same with no decay, no sustain and a sustain level of 1 (:304-321). */
	Audio apply_adsr_envelope( Second attack_time, Second decay_time, Second sustain_time, Second release_time, Amplitude sustain_level,
		float attack_exponent = 1, float decay_exponent = 1, float release_exponent = 1 ) const;
	Audio apply_ar_envelope( Second attack_time, Second release_time, float attack_exponent = 1, float release_exponent = 1 ) const;

	// ---- filters ----
	/** The Butterworth low-pass of any order with a cutoff that may change every frame (Audio/AudioFilter.cpp:327-378; Zavalishin, The
	 *  Art of VA Filter Design, 8.6), on the device (flanhip_filter_1pole_dev): for an odd order a 1-pole TPT section first,
	 *  then order / 2 2-pole state-variable sections, each a scan over the frames.  cutoff is sampled once per frame at f * frame_to_time( 1 )
	 *  and clamped to [1, sample rate / 2]; a constant samples nothing.  Order 0 is a copy.  A null *this gives a null Audio.  The result
	 *  stays device-resident until read. */
	Audio filter_1pole_lowpass( const Function<Second, Frequency> & cutoff, uint16_t order = 1 ) const;
	/** The Butterworth high-pass (:380-387): the same cascade with every section's high output.  Order 0 is a copy. */
	Audio filter_1pole_highpass( const Function<Second, Frequency> & cutoff, uint16_t order = 1 ) const;
	/** { low, high } around one cutoff (:389-425): order <= 1 gives { filter_1pole_lowpass( 1 ), filter_1pole_highpass( 1 ) }, a higher
	 *  order each filter applied twice, { low( N ).low( N ), high( N ).high( N ) }.  The cutoff is sampled ONCE and the device curve serves
	 *  all calls.  Order 0 behaves as order 1.  A null *this gives two null Audios, as the reference's calls on it do. */
	std::vector<Audio> filter_1pole_split( const Function<Second, Frequency> & cutoff, uint16_t order = 1 ) const;
	/** The same 1-pole low-pass `repeats` times over (:280-316; the atmospheric scattering of the spatialisers).  No repeats give SILENCE of
	 *  this Audio's format, not a copy: the reference's loop never writes its zero-initialised output. */
	Audio filter_1pole_repeat_low( const Function<Second, Frequency> & cutoff, const uint16_t repeats ) const;
	/** The same 1-pole high-pass `repeats` times over (:318-324).  No repeats give silence. */
	Audio filter_1pole_repeat_high( const Function<Second, Frequency> & cutoff, const uint16_t repeats ) const;
	/** The Butterworth low shelf: the tilt of `gain` times amp( gain / 2 ) (Audio/AudioFilter.cpp:431-500; The Art of VA Filter Design, 10.2),
	 *  on the device (flanhip_filter2_dev).  cutoff and gain are sampled once per frame at f * ( 1.0f / sample rate ); a constant
	 *  samples nothing.  The cutoff is clamped to [1, sample rate / 2] BEFORE it is scaled by M = amp( gain / ( 2 order ) ).  Kept quirks: the
	 *  2-pole sections run with R = Re( pole ) / w, negative and tiny, so from order 2 on the filter is mildly unstable (order 4 puts out
	 *  x 1000); order 0 is a copy times amp( gain / 2 ).  A null *this gives a null Audio.  The result stays device-resident. */
	Audio filter_1pole_lowshelf( const Function<Second, Frequency> & cutoff, const Function<Second, Decibel> & gain, uint16_t order = 1 ) const;
	/** The Butterworth high shelf (:502-512): the tilt of -gain times amp( gain / 2 ).  The quirks of filter_1pole_lowshelf. */
	Audio filter_1pole_highshelf( const Function<Second, Frequency> & cutoff, const Function<Second, Decibel> & gain, uint16_t order = 1 ) const;

	/** The resonant low-pass of order N: a Butterworth filter whose every pole is split in two by the damping (:520-592; 10.4), N
	 *  state-variable sections with a per-frame cutoff and damping, each a scan over the frames (flanhip_filter2_dev).  cutoff
	 *  and damping are sampled once per frame at f * ( 1.0f / sample rate ); a constant samples nothing.  The cutoff is clamped to [1, sample
	 *  rate / 2], the damping is not.  Kept quirks: a damping above 1 at a frame makes acos( damping ) NaN, so every ODD order, order 1 included,
	 *  puts out NaN from that frame on (even orders are fine); order 0 is a copy.  A null *this gives a null Audio.  The result stays
	 *  device-resident until read. */
	Audio filter_2pole_lowpass( const Function<Second, Frequency> & cutoff, const Function<Second, float> & damping, uint16_t order = 1 ) const;
	/** The band-pass (:594-602): every section's bp * 2 * R with the section's own R.  The quirks of filter_2pole_lowpass. */
	Audio filter_2pole_bandpass( const Function<Second, Frequency> & cutoff, const Function<Second, float> & damping, uint16_t order = 1 ) const;
	/** The high-pass (:604-612).  The quirks of filter_2pole_lowpass. */
	Audio filter_2pole_highpass( const Function<Second, Frequency> & cutoff, const Function<Second, float> & damping, uint16_t order = 1 ) const;
	/** The input minus the band-pass, ( 0 + ( -band ) ) + x per sample (:614-624).  The quirks of filter_2pole_lowpass, and order 0 is
	 *  SILENCE: the band-pass of order 0 is a copy. */
	Audio filter_2pole_notch( const Function<Second, Frequency> & cutoff, const Function<Second, float> & damping, uint16_t order = 1 ) const;
	/** The resonant low shelf (:709-724; 10.4): M = amp( ( gain / 2 ) / ( 2 order ) ), the sections of filter_2pole_lowpass at cutoff * M, each
	 *  putting out lp / M^4 + band / M^2 + hp.  gain is sampled at f * ( 1.0f / sample rate ), but cutoff and damping at frame_to_time( f ) =
	 *  f / sample rate (:648-654) -- not always the same float.  Kept quirks: the cutoff is NOT clamped; a damping above 1 makes odd orders NaN
	 *  from that frame on; order 0 is a copy.  A null *this gives a null Audio.  The result stays device-resident. */
	Audio filter_2pole_lowshelf( const Function<Second, Frequency> & cutoff, const Function<Second, float> & damping,
		const Function<Second, Decibel> & gain, uint16_t order = 1 ) const;
	/** The band shelf (:726-740): M = amp( -gain / ( 2 order ) ), the cutoff as it is and the damping times M, each section putting out
	 *  lp + band / M^2 + hp.  The quirks of filter_2pole_lowshelf, and damping * M can pass 1 where the damping does not: odd orders go NaN. */
	Audio filter_2pole_bandshelf( const Function<Second, Frequency> & cutoff, const Function<Second, float> & damping,
		const Function<Second, Decibel> & gain, uint16_t order = 1 ) const;
	/** The high shelf (:742-758): as the low shelf, each section putting out lp + band * M^2 + hp * M^4.  The quirks of filter_2pole_lowshelf. */
	Audio filter_2pole_highshelf( const Function<Second, Frequency> & cutoff, const Function<Second, float> & damping,
		const Function<Second, Decibel> & gain, uint16_t order = 1 ) const;

	/** The feedback comb (Audio/AudioFilter.cpp:988-1043; The Art of VA Filter Design, 11.5-11.6): u[n] = x[n] + feedback f u[p], out =
	 *  wet_dry u[n] + ( 1 - wet_dry ) f u[p], f = invert ? -1 : 1, with the delay of half a period of the cutoff, p = trunc( n - sample rate /
	 *  ( 2 cutoff ) ), changing every frame; on the device the links are followed by pointer jumping in fp64 (flanhip_filter_comb_dev; DESIGN.md
	 *  4.18).  cutoff, feedback and wet_dry are sampled once per frame at f * ( 1.0f / sample rate ); a constant samples nothing.  The cutoff
	 *  is clamped to [1, sample rate / 2], the feedback is not.  Kept quirks: the delay is truncated toward zero, so a read from between frame
	 *  -1 and frame 0 reads frame 0, and a fractional delay d is n - trunc( n - d ) frames; a read outside the signal reads 0; a NaN cutoff
	 *  at a frame reads 0 there.  The result is within 1 fp32 ulp of the exact recurrence, not bit-identical to the reference's fp32 loop
	 *  unless the feedback is 0.  A feedback above 1 in magnitude is promised only while its product along a chain of reads stays in fp64's
	 *  range.  A null *this gives a null Audio.  The result stays device-resident until read. */
	Audio filter_comb( const Function<Second, Frequency> & cutoff, const Function<Second, float> & feedback = 0, const Function<Second, float> & wet_dry = .5,
		bool invert = false ) const;

	/** The 1-pole multinotch (Audio/AudioFilter.cpp:802-885; The Art of VA Filter Design, 11.2, 11.6): `order` 1-pole all-pass sections in a
	 *  row with an instantaneous feedback path around them, x_bar = x + inv feedback allpass^order( x_bar ) solved in closed form per frame,
	 *  out = wet_dry x_bar + ( 1 - wet_dry ) inv allpass^order( x_bar ), inv = invert ? -1 : 1: at wet_dry .5 a notch at every other multiple
	 *  of pi of the cascade's phase.  On the device a frame is a dense map of the `order` states and the frames are a scan of such maps
	 *  (flanhip_multinotch_dev); the result is within the reference's own fp32 rounding of the exact loop, not bit-identical
	 *  to it.  cutoff, feedback and wet_dry are sampled once per frame at f * ( 1.0f / sample rate ); a constant samples nothing.  The cutoff
	 *  is clamped to [1, sample rate / 2] and prewarped; the feedback is not clamped, | feedback | < 1 is the stable range.  NOT offered:
	 *  use_saturator == true (a Newton iteration on tanh per frame, no scan), order 0 (undefined in the reference) and orders above 16: each
	 *  gives a message and a null Audio.  A null *this gives a null Audio.  The result stays device-resident until read. */
	Audio filter_1pole_multinotch( uint16_t order, const Function<Second, Frequency> & cutoff, const Function<Second, float> & feedback = 0, bool invert = false,
		const Function<Second, float> & wet_dry = .5, bool use_saturator = false ) const;
	/** The 2-pole multinotch (:887-986): as the 1-pole one with `order` state-variable sections, each putting out lp - 2 damping bp + hp, whose
	 *  damping is sampled per frame like the rest and is not clamped.  Orders 1 ... 8 (16 states). */
	Audio filter_2pole_multinotch( uint16_t order, const Function<Second, Frequency> & cutoff, const Function<Second, float> & damping,
		const Function<Second, float> & feedback = 0, bool invert = false, const Function<Second, float> & wet_dry = .5, bool use_saturator = false ) const;

	// ---- single sideband ----
	/** The signal's positive spectrum alone -- an approximate Hilbert transform by a phase-difference network -- times a complex modulator, real
	 *  part (Audio/AudioFilter.cpp:1162-1186): spectral convolution with one sideband, so a complex sinusoid shifts every frequency.  The
	 *  network (:1045-1160) is two cascades of ten 1-pole all-pass sections whose outputs are 90 degrees apart from 50 Hz to 15 kHz; both
	 *  cascades and the product run in one pass on the device (flanhip_halfband_modulate_dev).  Per frame
	 *  out = first * re - second * im, three fp32 roundings.  Kept quirks: the poles come from phase_diff_network_pole_design( 20, 5, 22000 )
	 *  whatever the sample rate and are used as they are, no prewarp and no clamp; the FIRST cascade has the odd-indexed poles of the design;
	 *  nothing is anti-aliased.  modulator is sampled once per frame at f * ( 1.0f / sample rate ); a constant samples nothing.  A null *this
	 *  gives a null Audio.  The result stays device-resident until read. */
	Audio halfband_modulate( const Function<Second, std::complex<float>> & modulator ) const;
	/** The Bode frequency shifter (:1188-1227): every frequency moved by shift( t ) Hz, up or down.  First filter_1pole_lowpass( 8 ) at sample
	 *  rate / 2 - 1000 less a positive shift and filter_1pole_highpass( 8 ) at low_cutoff plus a negative one, so that nothing is moved past
	 *  Nyquist or below 0; then halfband_modulate with exp( i phase ).  shift is sampled once per frame (a constant samples nothing).  Kept
	 *  quirks: phase is the SEQUENTIAL fp32 running sum of shift * pi2 / sample rate from 0.0f and loses precision over long signals as the
	 *  reference's does; the filters' cutoffs and the modulator read the sampled shift through frame -> time -> frame in fp32, which is the
	 *  identity below four million frames and off by one for some frames above; an index that lands on the frame count reads the last frame
	 *  (the reference reads out of bounds there).  A null *this gives a null Audio.  The result stays device-resident until read. */
	Audio shift_frequency( const Function<Second, Frequency> & shift, Frequency low_cutoff = 30 ) const;    // Audio.h:855
	/** halfband_modulate with another Audio as the modulator (:1229-1263): each operand through filter_1pole_lowpass( its sample rate / 2 -
	 *  2000, 8 ).filter_1pole_highpass( 30, 8 ) and the network at ITS OWN sample rate -- the modulator is not resampled --, then
	 *  out = a_first * b_first - a_second * b_second over the channels and frames both have (flanhip_halfband_multiply_dev: four cascades
	 *  and the product in one pass).  The result has this Audio's sample rate.  A null *this or a null modulator (which the reference
	 *  dereferences) gives a null Audio.  The result stays device-resident until read. */
	Audio halfband_multiply( const Audio & modulator ) const;

	// ---- channels ----
	/** Mono to stereo (Audio/AudioConversions.cpp:58-85): both channels the input / sqrt( 2.0f ), on the device (flanhip_audio_to_stereo_dev;
	 *  DESIGN.md 4.20).  A stereo input is copied; any other channel count prints the reference's message and gives two silent channels, as
	 *  the reference's zero-initialised output does.  A null *this gives a null Audio.  The result stays device-resident until read. */
	Audio convert_to_stereo() const;
	/** The mean over the channels (:87-104): the channels added in order in fp32, divided by their number (flanhip_audio_to_mono_dev). */
	Audio convert_to_mono() const;
	/** One mono Audio per channel (Audio/AudioChannels.cpp:13-29), device-to-device copies (flanhip_audio_copy_rows_dev).  A null *this gives
	 *  an empty vector. */
	std::vector<Audio> split_channels() const;
	/** All channels of all inputs in order (:31-67): the longest input's length, zeros behind the shorter ones, device-to-device copies.
	 *  Inputs of other sample rates are first resampled to the highest one (Audio::resample), all of them as the reference does.  No inputs,
	 *  a null pointer or a null Audio among them (which the reference does not guard against) give a null Audio. */
	static Audio combine_channels( const std::vector<const Audio *> & channels );
	static Audio combine_channels( const std::vector<Audio> & channels );
	template<typename ... Ts, typename = std::enable_if_t<( std::is_same_v<Ts, Audio> && ... )>>
	static Audio combine_channels( const Ts & ... ins )
		{
		std::vector<const Audio *> p_ins;
		( p_ins.push_back( &ins ), ... );
		return combine_channels( p_ins );
		}

	// ---- spatial ----
	/** Constant-power panning (Audio/AudioSpatial.cpp:9-40): channel 0 times sine2( p ), channel 1 times sine2( 1 - p ), p = pan_amount( t ) /
	 *  2.0f + 0.5f, sine2( x ) = sqrt( 2 ) sin( pi / 4 x ) (Interpolator::sine2 with the double sin the reference's compiler picks), on the
	 *  device (flanhip_audio_pan_dev).  pan_amount in [-1, 1] (at -1 channel 0 is silent, at 1 channel 1) is sampled once per frame at f * ( 1.0f / sample rate );
	 *  a constant samples nothing.  A mono input is first convert_to_stereo(); more than two channels and a null *this give a null Audio.  The
	 *  result stays device-resident until read. */
	Audio pan( const Function<Second, float> & pan_amount ) const;
	/** pan on *this (:21-40): anything but stereo is left as it is, a null *this prints "Null input".  Computes into a fresh block and takes
	 *  it over. */
	Audio & pan_in_place( const Function<Second, float> & pan_amount );
	/** convert_to_mid_side().pan( widen_amount ).convert_to_left_right() (:42-45) */
	Audio widen( const Function<Second, float> & widen_amount ) const;
	/** A mono source moving in the plane, heard by two ears head_width apart on the y axis, the left one at +y (:88-281).  Per ear: the input
	 *  blended with its filter_1pole_lowpass( 500, 1 ) by the angle between the source and the ear's axis (75 degrees off the nose), times
	 *  1 / ( distance + 0.00001 ), then delayed by distance / 343 seconds -- a delay that follows the source, so the ear hears Doppler: the
	 *  reference's WDL sinc resampler in feed mode, 32 taps, a new rate every 32 frames.  On the device (flanhip_spatial_ear_dev,
	 *  flanhip_spatial_itd_dev); sampling the Functions, the speed limiter and the resampler's block plan are host work.
	 *  position is sampled once per frame at f * ( 1.0f / sample rate ); unless it is a constant its speed is limited to clamp( speed_limit( t ),
	 *  0, 342 ) metres per second, a sequential recurrence in fp64.  A constant position is a pure delay of Frame( n + delay ) frames in all
	 *  (:139-153).  The result has two channels and the longer ear's length; the resampler is never flushed, so the last 17 to 33 input frames
	 *  are not heard.  A non-mono input prints the reference's message and gives a null Audio.  Where the reference makes a zero-frame Audio -- a
	 *  moving source and 32 frames or fewer -- this gives a null Audio and one line on std::cout, before anything is sampled: an Audio
	 *  without frames is a null Audio here.  The result stays device-resident until read. */
	Audio stereo_spatialize( const Function<Second, vec2> & position, Meter head_width = 0.18f,
		const Function<Second, float> & speed_limit = std::numeric_limits<float>::max() ) const;

	// ---- information ----
	/** The wavelength, in frames, of one window of one channel by the YIN method (Audio/AudioInformation.cpp:138-166): the cumulative-mean-
	 *  normalised difference function d' of the window_size samples from start (:18-75), its valleys with parabolic interpolation
	 *  (DSPUtility.cpp:37-147) and, among the valleys beyond minimum_wavelength, the first one within a factor 2 of the lowest, if it is below
	 *  absolute_cutoff; 0 where nothing is found.  On the device (flanhip_audio_local_wavelength_dev): d as the sum it is defined
	 *  as, not through the reference's fp32 FFTs, so results agree with the reference to its own accuracy, not bit for bit.  Kept quirk: on an
	 *  exactly periodic window the lowest valley's y is 0 or below, nothing is below twice that, and the answer is 0.  window_size up to 16384.
	 *  A null *this gives 0; so does a channel or window outside the signal, with one line on std::cerr. */
	float get_local_wavelength( Channel channel, Frame start, Frame window_size = 2048, float absolute_cutoff = 0.2f, Frame minimum_wavelength = 10 ) const;
	/** get_local_wavelength at start, start + hop, ... while frame + window_size < end (end == -1: the signal's end), all windows in one launch,
	 *  then the reference's octave-continuity pass on the host (:168-229): a doubling of the wavelength that lasts at most a tenth of a second
	 *  is halved; the first longer one ends the pass.  A null *this, no window, a raised canceller and arguments the device refuses give an
	 *  empty vector. */
	std::vector<float> get_local_wavelengths( Channel channel, Frame start = 0, Frame end = -1, Frame window_size = 2048, Frame hop = 128,
		float absolute_cutoff = 0.2f, Frame minimum_wavelength = 10, flan_CANCEL_ARG ) const;
	/** The mean of the non-zero wavelengths (:245-265), in fp32 on the host: -1 unless more than min_active_ratio of the entries differ from -1
	 *  (kept quirk: undetected windows are 0, not -1, so they count as active and are then left out of the mean), and -1 if max_length_sigma
	 *  != -1 and the standard deviation exceeds it.  A null *this gives 0. */
	float get_average_wavelength( const std::vector<float> & local_wavelengths, float min_active_ratio = 0, float max_length_sigma = -1 ) const;
	/** get_average_wavelength( get_local_wavelengths( channel, start, end, window_size, hop ), ... ) (:231-243) */
	float get_average_wavelength( Channel channel, float min_active_ratio = 0, float max_length_sigma = -1, Frame start = 0, Frame end = -1,
		Frame window_size = 2048, Frame hop = 128, flan_CANCEL_ARG ) const;
	/** sample rate / get_local_wavelength( channel, start, window_size, 0.2f, 10 ) (:267-270): infinity where no wavelength is found, as in
	 *  the reference. */
	Frequency get_local_frequency( Channel channel, Frame start = 0, Frame window_size = 2048, flan_CANCEL_ARG ) const;
	/** get_local_wavelengths( ..., 0.2f, 10 ) with every non-zero wavelength turned into sample rate / wavelength (:296-304); a 0 stays 0. */
	std::vector<Frequency> get_local_frequencies( Channel channel, Frame start = 0, Frame end = -1, Frame window_size = 2048, Frame hop = 128, flan_CANCEL_ARG ) const;
	/** convert_to_mono().get_local_frequencies( 0, 0, -1, 2048, 128 ) as a function of time, linear between the hops and 0 outside them
	 *  (:388-407).  Where the reference would read an empty vector (a null *this, a signal of 2048 frames or fewer) the function is 0. */
	Function<Second, Amplitude> get_frequency_envelope() const;
	/** The sum of every channel's squared samples (Audio/AudioInformation.cpp:121-129), on the device (flanhip_audio_energy_dev):
	 *  the squares exact in fp64, summed in fp64 in a fixed order without atomics, rounded to fp32 once.  That is the correctly rounded sum to
	 *  within one ulp, the same bits on every run -- not the rounding sequence of the reference's sequential fp32 loop.  A null *this gives an
	 *  empty vector. */
	std::vector<float> get_total_energy() const;
	/** mix( { this, other }, { 0, 0 }, { 1, -1 } ).get_total_energy(), other first resample()d to this sample rate if it differs (:131-136). */
	std::vector<float> get_energy_difference( const Audio & other ) const;
	/** The rectified mono signal smoothed by a Hann window window_width long, as a function of time (:320-363): convert_to_mono, a rectifier
	 *  (flanhip_audio_rectify_dev), convolve( window, false ) and the gain pi / 2 / ( the window's fp32 running sum ), all on the device; the
	 *  window is made on the host.  The Function owns the downloaded samples, is linear between frames and 0 outside [0, ( size - 1 ) / sr ).
	 *  A null *this, window_width <= 0 and a window of no frames give the constant 0. */
	Function<Second, Amplitude> get_amplitude_envelope( Second window_width = 0.1f ) const;

	// ---- cutting, mixing and granular synthesis ----
	// Everything below ends in one kernel (flanhip_grains_mix_dev): an output sample is the fp32 sum, in the order of the inputs,
	// of the inputs that cover it, bit for bit what the reference's loop over its inputs computes (Audio/AudioCombination.cpp:155-167); grains are
	// cut, faded and windowed while they are read and never written anywhere.  Results stay device-resident until read.  Not offered: select,
	// mix_in_place, texture_effect, synthesize_trainlets, synthesize_impulse.
	/** The frames between two times, with square-root fades at either end (Audio/AudioTemporal.cpp:190-234, Audio/AudioVolume.cpp:102-135): times
	 *  become frames by truncation; end <= start gives a null Audio, checked before start and end are clamped to [0, frames - 1] -- so the last
	 *  frame is never part of a cut --; fades are clamped at 0 and, where together they are longer than the cut, both scaled down and floored.  A
	 *  time no Frame holds (NaN, an infinity) gives a null Audio; so does a null *this. */
	Audio cut( Second start_time, Second end_time, Second start_fade = 0, Second end_fade = 0 ) const;
	Audio cut_frames( Frame start, Frame end, Frame start_fade = 0, Frame end_fade = 0 ) const;
	/** The sum of the inputs, input i from start_times[i] on and times amplitudes[i] (Audio/AudioCombination.cpp:78-179; the overloads of
	 *  Audio/Audio.h:876-908).  The longest of the three lists sets the number of terms: inputs loop, start times default to 0, amplitudes to 1.
	 *  Unless all sample rates are the highest one every input is first resample()d to it; the output has the widest channel count and
	 *  max( start frame + frames ) frames; what starts before time 0 loses its beginning.  A constant amplitude travels as a scalar; a callable one
	 *  is sampled on the host over the input's own frames at global time, f * frame_to_time( 1 ) for f in [start, start + frames).
	 *  No inputs give a null Audio.  Where the reference would read through a null pointer -- one among the inputs, or an amplitude -- the result
	 *  is a null Audio.  A null Audio OBJECT among the inputs adds nothing but counts with its start for the length, as in the reference; its sample
	 *  rate is not looked at, and if every input is one the result is a null Audio. */
	static Audio mix( std::vector<const Audio *> ins, std::vector<Second> start_times = {}, std::vector<Amplitude> amplitudes = {} );
	static Audio mix( const std::vector<Audio> & ins, std::vector<Second> start_times = {}, std::vector<Amplitude> amplitudes = {} );
	static Audio mix( std::vector<const Audio *> ins, std::vector<Second> start_times, const std::vector<const Function<Second, Amplitude> *> & amplitudes );
	static Audio mix( const std::vector<Audio> & ins, const std::vector<Second> & start_times, const std::vector<Function<Second, Amplitude>> & amplitudes );
	template<typename ... Ts, typename = std::enable_if_t<( std::is_same_v<Ts, Audio> && ... )>>
	static Audio mix( const Ts & ... ins )
		{
		std::vector<const Audio *> p_ins;
		( p_ins.push_back( &ins ), ... );
		return mix( p_ins );
		}
	/** The inputs tip to tail (:205-237): input i + 1 starts where input i ends plus offsets[i + 1]; offsets has one entry more than there are
	 *  inputs (the first and the last are not read), else the result is a null Audio.  Start-time arithmetic in fp32 over mix. */
	static Audio join( const std::vector<const Audio *> & ins, const std::vector<Second> & offsets );
	static Audio join( const std::vector<const Audio *> & ins, Second offset = 0 );
	static Audio join( const std::vector<Audio> & ins, Second offset = 0 );
	/** Grains made by the caller's function at the times an event rate decides, mixed in one launch (Audio/AudioSynthesis.cpp:310-398).
	 *  grains_per_second and time_scatter are sampled once per frame of `length` at f * ( 1.0f / sample_rate ) and clamped at 0; an event falls
	 *  where the running sum of rate / sample_rate passes an integer, the first at frame 0 (flanhip_grains_events).  time_scatter moves every event
	 *  by a normal deviate of scatter / rate seconds; the engine is seeded from the clock and a counter, as the reference's is from the clock.
	 *  grain_source runs on the calling thread in event order, whatever its policy: its device calls share one stream.  length <= 0 gives a
	 *  null Audio. */
	static Audio synthesize_grains( Second length, const Function<Second, float> & grains_per_second, const Function<Second, float> & time_scatter,
		const Function<Second, Audio> & grain_source, FrameRate sample_rate = 48000 );
	/** *this repeated at the events (:401-473).  Without a mod nothing is copied: every event reads *this.  With one, a copy per event goes through
	 *  mod( copy, event time ) first; with mod_feedback each copy is made from the event before's result.  The mod runs on the calling thread in
	 *  event order. */
	Audio texture( Second length, const Function<Second, float> & grains_per_second, const Function<Second, float> & time_scatter,
		const AudioMod & mod = AudioMod(), bool mod_feedback = false ) const;
	/** Granular resynthesis (:572-609): at each event time t a grain cut( selection( t ), selection( t ) + grain_length( t ), fade( t ), fade( t ) )
	 *  of *this is placed at t.  The three Functions are sampled over the frames of `length` at f * frame_to_time( 1 ) and read at the event's
	 *  frame.  Without a mod the grains are cut inside the mixing kernel: one launch over *this, nothing materialised.  With one, every grain is
	 *  cut on the device into an Audio of its own, handed to mod( grain, t ) on the calling thread in event order, and the results are mixed by
	 *  the same kernel; an identity mod gives the bits of the null mod.  If no grain has a frame the result is a null Audio. */
	Audio granulate( Second length, const Function<Second, float> & grains_per_second, const Function<Second, float> & time_scatter,
		const Function<Second, Second> & time_selection, const Function<Second, Second> & grain_length, const Function<Second, Second> & fade_time = 0,
		const AudioMod & mod = AudioMod() ) const;
	/** Pitch-synchronous overlap-add (:611-638): granulate at get_frequency_envelope()'s rate, grains two periods long with 0.05 s fades (which the
	 *  rescale shortens to half a grain each) under a Hann window over the grain's own length, read from time_selection( t ): a time stretch that
	 *  keeps the pitch.  Where no pitch is found the rate is 0 and the grain length 2.0f / 0: no grain.  Without a mod the window is applied in the
	 *  mixing kernel; a mod takes granulate's general path and the window follows it (modify_volume_in_place on the grain).  The window is
	 *  hann( x ) = 0.5f * ( 1.0f - cos( 2.0f * pi * x ) ) with the DOUBLE cos the reference's unqualified call picks (WindowFunctions.cpp:10-13). */
	Audio psola( Second length, const Function<Second, Second> & time_selection, const AudioMod & mod = AudioMod() ) const;
	/** A tone from the spectral dispersion and amplitude of each harmonic (Audio/AudioSynthesis.cpp:151-268): one period of 2^spectrum_size_power
	 *  frames at 48000 Hz made by ONE inverse real FFT over a spectrum whose bin near harmonic h of 2^fundamental_power Hz holds
	 *  peak_distribution( ( x - mean ) / sd ) / sd * harmonic_scale( h ) with sd = spread( h ) (the bin's own frequency where sd <= 0.001) at a
	 *  random phase, then read through the 64-tap sinc resampler at freq( t ), channel c starting c / num_channels of a period in, and set to volume 1.
	 *  spread and harmonic_scale are sampled once per harmonic, peak_distribution once per bin under its policy, freq at every output frame at
	 *  frame / 48000 (a block of `granularity` seconds reads the entry of its first frame); all of that on the host, the transform, the loop and
	 *  the normalisation on the device (flanhip_audio_synthesize_spectrum_dev).  `phases`: one angle per bin ( 2^(spectrum_size_power-1) + 1 of
	 *  them), which makes the call deterministic; without it they come from std::mt19937 seeded from std::random_device, drawn in ascending bin
	 *  order.  Bins without a harmonic, which the reference leaves uninitialised, are zero.  length <= 0, a power <= 0, fundamental_power >
	 *  spectrum_size_power or granularity <= 0 give a null Audio (:163-168); a size the library does not serve ( spectrum_size_power outside
	 *  6 ... 22 ) or a rate it refuses gives a null Audio and one line on std::cerr. */
	static Audio synthesize_spectrum( Second length, const Function<Second, Frequency> & freq,
		const Function<Harmonic, Frequency> & spread = []( Harmonic h ){ return Frequency( h ); },
		const Function<Harmonic, Amplitude> & harmonic_scale = []( Harmonic h ){ return 1.0f / std::sqrt( float( h ) ); },
		const Function<Frequency, Amplitude> & peak_distribution = []( Frequency x ){ return 1.0f / std::sqrt( pi2 ) * std::exp( -0.5f * std::pow( x, 2.0f ) ); },
		int fundamental_power = 8, int spectrum_size_power = 20, Channel num_channels = 2, Second granularity = 0.001f,
		const std::vector<Radian> * phases = nullptr );
	/** An oscillator (Audio/AudioSynthesis.cpp:25-69): wave( phase ) at oversample times the sample rate, phase the running sum of freq over the
	 *  oversampled frames modulo 1 cycle, then r8brain's chain down into exactly Frame( length * sample_rate ) frames, one channel.  freq is
	 *  sampled once per oversampled frame at i * ( 1.0f / ( sample_rate * oversample ) ); a constant travels as a scalar.  The phases are a scan
	 *  on the device carried in fp64 (flanhip_osc_phase_dev: within 2^-23 of a cycle of the exact modular sum; the reference's fp32 scan has no
	 *  defined grouping and drifts).  A named waveform is evaluated inside the scan and nothing leaves the device; any other is evaluated on the
	 *  host at the downloaded phases under its policy.  oversample 1 copies the wave samples, as r8brain does for equal rates.  oversample < 1,
	 *  length <= 0, sample_rate <= 0, no output frame, or more oversampled frames than a Frame counts give a null Audio. */
	static Audio synthesize_waveform( const Waveform & wave, Second length, const Function<Second, Frequency> & freq, FrameRate sample_rate = 48000,
		int oversample = 16 );
	/** Uniform noise in [-1, 1) drawn at oversample times the sample rate on the host -- std::mt19937( seed ) through
	 *  std::uniform_real_distribution<>( -1.0f, 1.0f ), :80-86 --, then resample( sample_rate ) (:71-89).  A seed names one result; the default
	 *  is random_seed(), as the reference seeds from std::random_device. */
	static Audio synthesize_white_noise( Second length, FrameRate sample_rate = 48000, int oversample = 16, uint64_t seed = random_seed() );

	// ---- silence removal and slicing (Audio/AudioTemporal.cpp:10-188, 301-546) ----
	// The loud chunks are found by one scan on the device (flanhip_loud_summary_dev, flanhip_loud_chunks_dev); the fades, splits and plans are
	// host arithmetic behind the C ABI; everything ends in the mixing kernel above, so without the Hann flag results are the reference's bit for
	// bit.  Not offered: texture_effect, select, mix_in_place, and the commented-out stereo_delay.
	/** What std::random_device gives: the default seed of rearrange and random_chunks, as the reference seeds its engines (:477, :522). */
	static uint64_t random_seed();
	/** *this with -start frames of silence put before it and end frames after it; negative amounts cut (:96-114 over mix_in_place,
	 *  AudioCombination.cpp:181-203): one event into a cleared output of -start + frames + end frames, placed at
	 *  Frame( time_to_frame( -frame_to_time( start ) ) ), the fp32 round trip included.  (The reference adds the float time_to_frame( start time )
	 *  to every source frame before it truncates, which lands elsewhere only where that round trip is inexact and start > 0.)  A result of
	 *  <= 0 frames and a null *this give a null Audio. */
	Audio modify_boundaries_frames( Frame start, Frame end ) const;
	Audio modify_boundaries( Second start, Second end ) const;
	/** The cut from the first to the last frame with a sample above non_silent_level in any channel, widened by fade_time on either side where
	 *  the signal has room and faded over it (:124-153).  The compare is signed, and false for a NaN.  The two frames come from the device's
	 *  summary.  Nothing noisy cuts from the last frame to frame 0: a null Audio unless the fade reaches over. */
	Audio remove_edge_silence( Amplitude non_silent_level, Second fade_time = 0 ) const;
	/** The stretches where some channel is above non_silent_level, each closed by more than minimum_gap of quiet, each widened by fade_in_time
	 *  and faded, with the reference's fade arithmetic and its quirks (:10-86, flanhip_loud_chunks_fades): a chunk that reaches the end loses its last
	 *  frame to cut_frames' clamp.  Every chunk is cut on the device.  A chunk that cuts to nothing -- one noisy frame and no fade -- is a null
	 *  Audio in the vector.  Nothing noisy, and a null *this, give an empty vector. */
	std::vector<Audio> get_loud_chunks( Amplitude non_silent_level, Second minimum_gap, Second fade_in_time = 0 ) const;
	/** join( get_loud_chunks( ... ), offsets -2 fade ) (:164-172) as ONE launch over *this: the scan, the fades plan, then one event per chunk read
	 *  from *this directly; no chunk is written.  A chunk that cuts to nothing is an empty event: it adds nothing and counts with its place for
	 *  the length alone, which is what mix does with a null Audio among its inputs.  remove_silence_unfused is the general path -- the chunks
	 *  made, then joined -- and gives the same bits. */
	Audio remove_silence( Amplitude non_silent_level, Second minimum_gap, Second fade_in_time = 0 ) const;
	Audio remove_silence_unfused( Amplitude non_silent_level, Second minimum_gap, Second fade_in_time = 0 ) const;
	/** out[c][f] = in[c][frames - 1 - f] (:174-188), on the device. */
	Audio reverse() const;
	/** *this num_iterations times, tip to tail with crossfade_time of overlap (:301-324).  Without a mod nothing is copied: every event reads
	 *  *this.  With one, iteration i is a copy gone through mod( copy, i * get_length() ), made from iteration i - 1's result under feedback; the mod
	 *  runs on the calling thread in order.  num_iterations < 1 gives a null Audio. */
	Audio iterate( int32_t num_iterations, Second crossfade_time = 0, const AudioMod & mod = AudioMod(), bool feedback = false ) const;
	/** A decaying echo (:326-361): texture( length + added_length, 1 / delay_time, 0, delay_mod, true ), where delay_mod leaves the event at
	 *  time 0 alone and gives every later one the user's mod and then one fp32 product per sample by decay at the event's time.  Both Functions are
	 *  sampled over the frames of the length at f * frame_to_time( 1 ); delay_time <= 0 gives a rate of 1 / sample rate. */
	Audio delay( Second added_length, const Function<Second, Second> & delay_time, const Function<Second, float> & decay = .5f, const AudioMod & mod = AudioMod() ) const;
	/** The pieces between the sorted split times, each cut_frames with `fade` at both ends (:409-438, flanhip_split_frames): times at or before
	 *  frame 0 are skipped and the first at or beyond the end stops the list.  split_with_lengths: the times are the fp32 running sum of the
	 *  lengths, negative ones counting as 0 (:440-451).  split_with_equal_lengths: ceil( length / slice_length ) equal lengths (:453-461);
	 *  slice_length <= 0 gives an empty vector.  Every piece loses the frame at frames - 1 if it reaches it (cut_frames' clamp). */
	std::vector<Audio> split_at_times( std::vector<Second> split_times, Second fade = 0 ) const;
	std::vector<Audio> split_with_lengths( std::vector<Second> split_lengths, Second fade = 0 ) const;
	std::vector<Audio> split_with_equal_lengths( Second slice_length, Second fade = 0 ) const;
	/** split_with_equal_lengths( slice_length + fade, fade ) without its last piece, in a random order, joined with -fade (:463-482), as one event
	 *  table over *this.  The order is flanhip_rearrange_order( pieces, seed ) -- a Fisher-Yates over std::mt19937 the library defines, where the
	 *  reference's std::shuffle is the standard library's own --, so a seed names one result.  Fewer than 2 pieces give a null Audio. */
	Audio rearrange( Second slice_length, Second fade = 0, uint64_t seed = random_seed() ) const;
	/** Chunks of *this from random places, chunk_length( t ) long, crossfaded over fade( t ), for `length` seconds (:484-546,
	 *  flanhip_random_chunks_plan).  Without a mod it is one event table over *this; with one every chunk is cut into an Audio, handed to
	 *  mod( chunk, its start time ) on the calling thread in order, and the results are joined.  The places come from std::mt19937( seed ). */
	Audio random_chunks( Second length, const Function<Second, Second> & chunk_length, const Function<Second, Second> & fade = 0,
		const AudioMod & mod = AudioMod(), uint64_t seed = random_seed() ) const;

	// the older camelCase spellings BASELINE.json's north_star uses
	PV convertToPV( Frame window_size = 2048, Frame hop = 128, Frame dft_size = 4096, flan_CANCEL_ARG ) const;
	};

} // namespace flan
