// Audio.cpp -- construction and conversions of flan::Audio over the C ABI
// (reference: src/flan/Audio/AudioConstructors.cpp, Conversions/AudioPV.cpp:12-84, Audio/AudioConversions.cpp:14-56,
// Audio/AudioCombination.cpp:299-352, Audio/AudioTemporal.cpp:236-299, Audio/AudioVolume.cpp (all of it),
// Audio/AudioFilter.cpp:280-758, 988-1263, Audio/AudioConversions.cpp:58-104, Audio/AudioChannels.cpp, Audio/AudioSpatial.cpp,
// Audio/AudioInformation.cpp:121-304, 320-407, Audio/AudioCombination.cpp:78-237, Audio/AudioTemporal.cpp:10-234, 301-546,
// Audio/AudioSynthesis.cpp:25-89, 310-473, 572-638).
#include "flan/Audio.h"

#include <algorithm>
#include <atomic>
#include <climits>
#include <cmath>
#include <ctime>
#include <iostream>
#include <random>

#include "device_call.h"
#include "flan/PV.h"

namespace flan {

namespace {
using detail::DeviceArg;
using detail::DeviceCall;

// A Function of time for the device (detail::DeviceArg): a constant goes as the scalar and samples nothing; a callable is sampled once per
// frame (Function::sample's arithmetic, Function.h:141-153) into a page-locked block and uploaded.  time_of( x ): the time frame x is sampled at
template<typename TimeOf>
DeviceArg upload_curve_at( const Function<Second, float> & fn, Frame n, TimeOf time_of )
	{
	if( fn.is_constant() ) return DeviceArg( fn.get_constant() );
	detail::StagingVector<float> sampled( size_t( std::max( n, 0 ) ) );
	detail::for_each_index( 0, n, fn.get_execution_policy(), [&]( int x ){ sampled[size_t( x )] = fn( time_of( x ) ); } );
	return DeviceArg::from_host( sampled.data(), sizeof( float ) * sampled.size(), "a sampled Function" );
	}

DeviceArg upload_curve( const Function<Second, float> & fn, Frame n, float scale )
	{
	return upload_curve_at( fn, n, [scale]( int x ){ return Second( x * scale ); } );
	}

// host values as a curve on the device
DeviceArg upload_values( const detail::StagingVector<float> & values )
	{
	return DeviceArg::from_host( values.data(), sizeof( float ) * values.size(), "a curve" );
	}

// what the skeleton could not make is the reference's null Audio, with its line on stdout
Audio or_null( AudioBuffer && out )
	{
	if( out.is_null() ) return Audio::create_null();
	return Audio( std::move( out ) );
	}

// One launch( out, ws ) into a fresh block of format f (detail::device_call)
template<typename Launch>
Audio audio_call( const char * who, const AudioBuffer::Format & f, bool have, size_t ws_bytes, Launch launch )
	{
	return or_null( detail::device_call<AudioBuffer, float>( who, f, size_t( f.num_channels ) * size_t( f.num_frames ), have, ws_bytes, launch ) );
	}

// What the three cascades below share: null in, null out (AudioFilter.cpp:287, :376, :385); a shape the C ABI refuses (no workspace) is a null
// too, before the data is asked onto the device; then one launch( d_x, out, ws ) over `me` into a fresh block of its format
template<typename Launch>
Audio cascade_call( const Audio & me, size_t ws_bytes, bool have, const char * who, Launch launch )
	{
	if( me.is_null() || ws_bytes == 0 ) return Audio::create_null();
	const float * d_x = me.device_data();
	if( !d_x ) return Audio::create_null();
	return audio_call( who, me.get_format(), have, ws_bytes, [&]( float * out, void * ws ){ return launch( d_x, out, ws ); } );
	}

// One cascade of flanhip_filter2_dev over `me` with its three arguments already on the device (or scalars)
Audio filter2_cascade( const Audio & me, const DeviceArg & cutoff, const DeviceArg & damping, const DeviceArg & gain, int kind, uint16_t order,
	const char * who )
	{
	return cascade_call( me, flanhip_filter2_workspace_bytes( me.get_num_channels(), me.get_num_frames() ), cutoff.ok && damping.ok && gain.ok, who,
		[&]( const float * d_x, float * out, void * ws )
		{
		return flanhip_filter2_dev( d_x, me.get_num_channels(), me.get_num_frames(), me.get_sample_rate(), cutoff.ptr(), cutoff.scalar,
			damping.ptr(), damping.scalar, gain.ptr(), gain.scalar, kind, int( order ), out, ws, nullptr );
		} );
	}

// One cascade of flanhip_filter_1pole_dev over `me` with a cutoff already on the device (or a scalar)
Audio filter_cascade( const Audio & me, const DeviceArg & cutoff, int kind, uint16_t order, const char * who )
	{
	return cascade_call( me, flanhip_filter_1pole_workspace_bytes( me.get_num_channels(), me.get_num_frames() ), cutoff.ok, who,
		[&]( const float * d_x, float * out, void * ws )
		{
		return flanhip_filter_1pole_dev( d_x, me.get_num_channels(), me.get_num_frames(), me.get_sample_rate(), cutoff.ptr(), cutoff.scalar, kind, int( order ), out, ws, nullptr );
		} );
	}

// flanhip_halfband_modulate_dev over `me` with the modulator already on the device (re and im, or the phase that stands for both)
Audio halfband_modulated( const Audio & me, const DeviceArg & re, const DeviceArg & im, const DeviceArg * phase, const char * who )
	{
	return cascade_call( me, flanhip_halfband_workspace_bytes( me.get_num_channels(), me.get_num_frames() ), re.ok && im.ok && ( !phase || ( phase->ok && phase->ptr() ) ), who,
		[&]( const float * d_x, float * out, void * ws )
		{
		return flanhip_halfband_modulate_dev( d_x, me.get_num_channels(), me.get_num_frames(), me.get_sample_rate(), re.ptr(), re.scalar,
			im.ptr(), im.scalar, phase ? phase->ptr() : nullptr, out, ws, nullptr );
		} );
	}

} // namespace

Audio::Audio() : AudioBuffer() {}
Audio::Audio( AudioBuffer && other ) : AudioBuffer( std::move( other ) ) {}
Audio Audio::copy() const { return AudioBuffer::copy(); }

Audio Audio::create_null()
	{
	std::cout << "Null Audio created";                        // AudioConstructors.cpp:19-23
	return Audio();
	}

Audio Audio::create_from_buffer( std::vector<float> && buffer, Channel num_channels, FrameRate sr )
	{
	return AudioBuffer( std::move( buffer ), num_channels, sr );
	}

Audio Audio::create_from_format( const AudioBuffer::Format & other ) { return AudioBuffer( other ); }

Audio Audio::create_empty_with_length( Second length, Channel num_channels, FrameRate sample_rate )
	{
	return create_empty_with_frames( Frame( length * sample_rate ), num_channels, sample_rate );
	}

Audio Audio::create_empty_with_frames( Frame num_frames, Channel num_channels, FrameRate sample_rate )
	{
	AudioBuffer::Format f;
	f.num_channels = num_channels; f.num_frames = num_frames; f.sample_rate = sample_rate;
	Audio out( ( AudioBuffer( f ) ) );
	out.clear_buffer();
	return out;
	}

PV Audio::convert_to_PV( Frame window_size, Frame hop, Frame dft_size, flan_CANCEL_ARG_CPP ) const
	{
	if( is_null() || hop < 1 || window_size < 2 ) return PV();
	if( canceller ) return PV();                               // flan_CANCEL_POINT( PV() ), AudioPV.cpp:49
	PVBuffer::Format f;                                        // AudioPV.cpp:20-27
	f.num_channels = get_num_channels();
	f.num_frames = Frame( flanhip_num_pv_frames( get_num_frames(), hop ) );
	f.num_bins = dft_size / 2 + 1;
	f.sample_rate = get_sample_rate();
	f.analysis_rate = get_sample_rate() / hop;
	f.window_size = window_size;

	const float * d_audio = device_data();
	if( !d_audio ) return PV();
	DeviceCall call( "convert_to_PV" );
	flanhip_MF * d_pv = call.output<flanhip_MF>( size_t( f.num_channels ) * f.num_frames * f.num_bins );
	if( !d_pv ) return PV();
	if( canceller ) return PV();
	// fused round trip: with a workspace the analysis kernel also leaves what convert_to_audio's pre-pass would compute (flanhip.h)
	void * ws = call.workspace( flanhip_synthesize_workspace_bytes( f.num_channels, f.num_frames, f.num_bins, f.sample_rate, f.analysis_rate, f.window_size ), true );
	const bool launched = call.launch( ws
		? flanhip_analyze_dev_fused( d_audio, f.num_channels, get_num_frames(), get_sample_rate(), window_size, hop, dft_size, d_pv, ws, nullptr )
		: flanhip_analyze_dev( d_audio, f.num_channels, get_num_frames(), get_sample_rate(), window_size, hop, dft_size, d_pv, nullptr ) );
	if( !launched ) return PV();
	// flan_CANCEL_POINT while the kernels run: the flag is polled during the wait and stops the launch (flanhip_wait_cancellable_fn)
	if( call.wait( canceller ) == FLANHIP_ERR_CANCELLED || canceller ) return PV();
	return call.finish_fused<PVBuffer>( f );
	}

PV Audio::convertToPV( Frame window_size, Frame hop, Frame dft_size, flan_CANCEL_ARG_CPP ) const
	{
	return convert_to_PV( window_size, hop, dft_size, canceller );
	}

PV Audio::convert_to_ms_PV( Frame window_size, Frame hop, Frame dft_size, flan_CANCEL_ARG_CPP ) const
	{
	if( get_num_channels() != 2 ) return PV();                 // AudioPV.cpp:82
	return convert_to_mid_side().convert_to_PV( window_size, hop, dft_size, canceller );
	}

Audio Audio::convert_to_mid_side() const
	{
	if( is_null() ) return Audio::create_null();
	if( get_num_channels() != 2 )
		{
		std::cout << "Can't transform non-stereo Audio between Mid-Side and Left-Right formats." << std::endl;   // AudioConversions.cpp:38
		return copy();
		}
	const float * d_in = device_data();
	if( !d_in ) return Audio::create_null();
	return audio_call( "convert_to_mid_side", get_format(), true, detail::kNoWorkspace, [&]( float * out, void * )
		{ return flanhip_mid_side_dev( d_in, get_num_frames(), out, nullptr ); } );
	}

Audio Audio::convert_to_left_right() const { return convert_to_mid_side(); }   // AudioConversions.cpp:53-56

Audio Audio::resample( FrameRate new_sample_rate ) const
	{
	if( is_null() ) return Audio::create_null();
	if( new_sample_rate == get_sample_rate() ) return copy();  // AudioConversions.cpp:18-19
	AudioBuffer::Format f = get_format();                      // :21-23
	f.num_frames = Frame( flanhip_resample_out_frames( get_num_frames(), get_sample_rate(), new_sample_rate ) );
	f.sample_rate = new_sample_rate;
	if( f.num_frames <= 0 ) return Audio::create_null();
	const float * d_in = device_data();
	// r8brain CDSPResampler with default parameters, one stream over the whole buffer (:25-27), whatever chain of stages it builds for the two rates
	return audio_call( "resample", f, d_in != nullptr, detail::kNoWorkspace, [&]( float * out, void * )
		{ return flanhip_resample_dev( d_in, get_num_channels(), get_num_frames(), get_sample_rate(), new_sample_rate, out, nullptr ); } );
	}

Audio Audio::convolve( const Audio & ir, bool normalize ) const
	{
	if( is_null() ) return Audio::create_null();                // AudioCombination.cpp:304-305
	if( ir.is_null() ) return Audio::create_null();
	// :307-308: an IR of another rate is resampled to this one first (all its channels as one stream, Audio::resample)
	const Audio resampled = get_sample_rate() == ir.get_sample_rate() ? Audio() : ir.resample( get_sample_rate() );
	const Audio & h = get_sample_rate() == ir.get_sample_rate() ? ir : resampled;
	if( h.is_null() ) return Audio::create_null();
	AudioBuffer::Format f = get_format();                        // :310-313
	f.num_frames = Frame( flanhip_convolve_out_frames( get_num_frames(), h.get_num_frames() ) );
	const size_t ws_bytes = flanhip_convolve_workspace_bytes( get_num_channels(), get_num_frames(), h.get_num_channels(), h.get_num_frames() );
	if( f.num_frames <= 0 || ws_bytes == 0 )
		{
		std::cerr << "flan: convolve refused the shape: " << get_num_channels() << " x " << get_num_frames() << " with "
		          << h.get_num_channels() << " x " << h.get_num_frames() << std::endl;
		return Audio::create_null();
		}
	const float * d_x = device_data();
	const float * d_h = h.device_data();
	if( !d_x || !d_h ) return Audio::create_null();
	return audio_call( "convolve", f, true, ws_bytes, [&]( float * out, void * ws )
		{ return flanhip_convolve_dev( d_x, get_num_channels(), get_num_frames(), d_h, h.get_num_channels(), h.get_num_frames(), get_sample_rate(), normalize ? 1 : 0, out, ws, nullptr ); } );
	}

Audio Audio::repitch( const Function<Second, float> & factor, Second granularity, WDLResampleType quality ) const
	{
	if( is_null() ) return Audio::create_null();                // AudioTemporal.cpp:238
	if( quality == WDLResampleType::Linear )
		{
		std::cout << "Audio::repitch: the Linear quality is not built (Sinc and Uninterpolated are)." << std::endl;
		return Audio();
		}
	Frame g = Frame( time_to_frame( granularity ) );            // :241-242
	if( g < 1 ) g = 1;
	const int count = int( std::ceil( get_num_frames() / float( g ) ) );       // :245
	const auto sampled = factor.sample( 0, count, granularity );
	std::vector<float> inv( size_t( std::max( count, 0 ) ) );
	for( size_t i = 0; i < inv.size(); ++i )                     // :246-249, in fp32
		{
		const float v = sampled.is_constant() ? sampled.get_constant() : sampled.get_vector()[i];
		inv[i] = std::clamp( 1.0f / v, 1.0f / 1000.0f, 1000.0f );
		}
	const int q = quality == WDLResampleType::Sinc ? FLANHIP_REPITCH_SINC : FLANHIP_REPITCH_UNINTERPOLATED;
	AudioBuffer::Format f = get_format();                        // :252-256
	f.num_frames = Frame( flanhip_audio_repitch_out_frames( inv.data(), int64_t( inv.size() ), g ) );
	const size_t ws_bytes = flanhip_audio_repitch_workspace_bytes( get_num_frames(), get_sample_rate(), inv.data(), int64_t( inv.size() ), g, q );
	if( f.num_frames <= 0 || ws_bytes == 0 )
		{
		std::cerr << "flan: repitch refused: " << get_num_channels() << " x " << get_num_frames() << ", granularity " << g << " frames: ";
		if( f.num_frames <= 0 ) std::cerr << "no output frames";              // (the length function sets no error text)
		else std::cerr << flanhip_last_error();
		std::cerr << std::endl;
		return Audio::create_null();
		}
	const float * d_x = device_data();
	if( !d_x ) return Audio::create_null();
	return audio_call( "repitch", f, true, ws_bytes, [&]( float * out, void * ws )
		{ return flanhip_audio_repitch_dev( d_x, get_num_channels(), get_num_frames(), get_sample_rate(), inv.data(), int64_t( inv.size() ), g, q, out, ws, nullptr ); } );
	}

Audio Audio::modify_volume( const Function<Second, float> & gain ) const
	{
	if( is_null() ) return Audio::create_null();                // AudioVolume.cpp:9
	const float * d_x = device_data();
	if( !d_x ) return Audio::create_null();
	const DeviceArg g = upload_curve( gain, get_num_frames(), 1.0f / get_sample_rate() );     // :36
	return audio_call( "modify_volume", get_format(), g.ok, detail::kNoWorkspace, [&]( float * out, void * )
		{ return flanhip_audio_gain_dev( d_x, get_num_channels(), get_num_frames(), g.ptr(), g.scalar, out, nullptr ); } );
	}

// the in-place forms compute into a fresh block and take it over: the block under *this may be shared (device_block())
Audio & Audio::modify_volume_in_place( const Function<Second, float> & gain )
	{
	if( is_null() ) return *this;
	Audio out = modify_volume( gain );
	if( !out.is_null() ) *this = std::move( out );
	return *this;
	}

Audio Audio::set_volume( const Function<Second, Amplitude> & level ) const
	{
	if( is_null() ) return Audio::create_null();                // :50
	const float * d_x = device_data();
	if( !d_x ) return Audio::create_null();
	const DeviceArg l = upload_curve( level, get_num_frames(), 1.0f / get_sample_rate() );
	// :63-66: the maximum, the m == 0 case and level( t ) / m are the device's (and so is the refusal of a shape: no 0 bytes reach the skeleton)
	const size_t ws_bytes = std::max<size_t>( flanhip_audio_set_volume_workspace_bytes( get_num_channels(), get_num_frames() ), 1 );
	return audio_call( "set_volume", get_format(), l.ok, ws_bytes, [&]( float * out, void * ws )
		{ return flanhip_audio_set_volume_dev( d_x, get_num_channels(), get_num_frames(), get_sample_rate(), l.ptr(), l.scalar, out, ws, nullptr ); } );
	}

Audio & Audio::set_volume_in_place( const Function<Second, Amplitude> & level )
	{
	if( is_null() ) return *this;                               // :60
	Audio out = set_volume( level );
	if( !out.is_null() ) *this = std::move( out );
	return *this;
	}

Audio Audio::compress( const Function<Second, Decibel> & threshold, const Function<Second, float> & compression_ratio,
	const Function<Second, Second> & attack, const Function<Second, Second> & release, const Function<Second, Decibel> & knee_width,
	const Audio * sidechain_source ) const
	{
	if( is_null() ) return Audio::create_null();                // :205
	const Audio & side = sidechain_source ? *sidechain_source : *this;     // :207-208
	if( side.is_null() ) return Audio::create_null();
	if( side.get_num_frames() < get_num_frames() )
		{
		std::cout << "Audio::compress: the sidechain has fewer frames than the Audio it controls." << std::endl;
		return Audio::create_null();
		}
	const size_t ws_bytes = flanhip_compress_workspace_bytes( get_num_frames() );
	if( ws_bytes == 0 ) return Audio::create_null();
	const float * d_x = device_data();
	const float * d_side = side.device_data();
	if( !d_x || !d_side ) return Audio::create_null();
	const float step = frame_to_time( 1 );                       // :220-224
	const DeviceArg t = upload_curve( threshold, get_num_frames(), step ), r = upload_curve( compression_ratio, get_num_frames(), step ),
		a = upload_curve( attack, get_num_frames(), step ), rel = upload_curve( release, get_num_frames(), step ),
		k = upload_curve( knee_width, get_num_frames(), step );
	return audio_call( "compress", get_format(), t.ok && r.ok && a.ok && rel.ok && k.ok, ws_bytes, [&]( float * out, void * ws )
		{
		return flanhip_compress_dev( d_x, get_num_channels(), get_num_frames(), get_sample_rate(), d_side, side.get_num_channels(), side.get_num_frames(),
			t.ptr(), t.scalar, r.ptr(), r.scalar, a.ptr(), a.scalar, rel.ptr(), rel.scalar, k.ptr(), k.scalar, out, nullptr, ws, nullptr );
		} );
	}

// :119, :291, :342: sample_function_over_domain is the Function sampled once per frame at f * frame_to_time( 1 ); the clamp is the device's
Audio Audio::filter_1pole_lowpass( const Function<Second, Frequency> & cutoff, uint16_t order ) const
	{
	if( is_null() || !device_data() ) return Audio::create_null();     // :376; without a device nothing is sampled
	return filter_cascade( *this, upload_curve( cutoff, get_num_frames(), frame_to_time( 1 ) ), FLANHIP_FILTER_BUTTERWORTH_LOW, order, "filter_1pole_lowpass" );
	}

Audio Audio::filter_1pole_highpass( const Function<Second, Frequency> & cutoff, uint16_t order ) const
	{
	if( is_null() || !device_data() ) return Audio::create_null();     // :385; without a device nothing is sampled
	return filter_cascade( *this, upload_curve( cutoff, get_num_frames(), frame_to_time( 1 ) ), FLANHIP_FILTER_BUTTERWORTH_HIGH, order, "filter_1pole_highpass" );
	}

std::vector<Audio> Audio::filter_1pole_split( const Function<Second, Frequency> & cutoff, uint16_t order ) const
	{
	std::vector<Audio> outs;
	if( is_null() || !device_data() ) { outs.push_back( Audio::create_null() ); outs.push_back( Audio::create_null() ); return outs; }
	// :401-404: the cutoff is sampled once; the reference's round( time_to_frame( t ) ) indexing hands the sampled curve itself to every call
	const DeviceArg c = upload_curve( cutoff, get_num_frames(), frame_to_time( 1 ) );
	const uint16_t n = order <= 1 ? uint16_t( 1 ) : order;     // :406-412
	Audio low = filter_cascade( *this, c, FLANHIP_FILTER_BUTTERWORTH_LOW, n, "filter_1pole_split" );
	Audio high = filter_cascade( *this, c, FLANHIP_FILTER_BUTTERWORTH_HIGH, n, "filter_1pole_split" );
	if( order > 1 )                                             // :414-422
		{
		low = filter_cascade( low, c, FLANHIP_FILTER_BUTTERWORTH_LOW, n, "filter_1pole_split" );
		high = filter_cascade( high, c, FLANHIP_FILTER_BUTTERWORTH_HIGH, n, "filter_1pole_split" );
		}
	outs.push_back( std::move( low ) );
	outs.push_back( std::move( high ) );
	return outs;
	}

Audio Audio::filter_1pole_repeat_low( const Function<Second, Frequency> & cutoff, const uint16_t repeats ) const
	{
	if( is_null() || !device_data() ) return Audio::create_null();     // :287
	return filter_cascade( *this, upload_curve( cutoff, get_num_frames(), frame_to_time( 1 ) ), FLANHIP_FILTER_REPEAT_LOW, repeats, "filter_1pole_repeat_low" );
	}

Audio Audio::filter_1pole_repeat_high( const Function<Second, Frequency> & cutoff, const uint16_t repeats ) const
	{
	if( is_null() || !device_data() ) return Audio::create_null();
	return filter_cascade( *this, upload_curve( cutoff, get_num_frames(), frame_to_time( 1 ) ), FLANHIP_FILTER_REPEAT_HIGH, repeats, "filter_1pole_repeat_high" );
	}

// :533-535: cutoff and damping through sample_function_over_domain, at f * ( 1.0f / sr ); the clamp and everything after it are the device's
static Audio filter_2pole( const Audio & me, const Function<Second, Frequency> & cutoff, const Function<Second, float> & damping, int kind,
	uint16_t order, const char * who )
	{
	if( me.is_null() || !me.device_data() ) return Audio::create_null();     // :590; without a device nothing is sampled
	const float step = me.frame_to_time( 1 );
	return filter2_cascade( me, upload_curve( cutoff, me.get_num_frames(), step ), upload_curve( damping, me.get_num_frames(), step ), DeviceArg(),
		kind, order, who );
	}

Audio Audio::filter_2pole_lowpass( const Function<Second, Frequency> & cutoff, const Function<Second, float> & damping, uint16_t order ) const
	{
	return filter_2pole( *this, cutoff, damping, FLANHIP_FILTER2_LOW, order, "filter_2pole_lowpass" );
	}

Audio Audio::filter_2pole_bandpass( const Function<Second, Frequency> & cutoff, const Function<Second, float> & damping, uint16_t order ) const
	{
	return filter_2pole( *this, cutoff, damping, FLANHIP_FILTER2_BAND, order, "filter_2pole_bandpass" );
	}

Audio Audio::filter_2pole_highpass( const Function<Second, Frequency> & cutoff, const Function<Second, float> & damping, uint16_t order ) const
	{
	return filter_2pole( *this, cutoff, damping, FLANHIP_FILTER2_HIGH, order, "filter_2pole_highpass" );
	}

Audio Audio::filter_2pole_notch( const Function<Second, Frequency> & cutoff, const Function<Second, float> & damping, uint16_t order ) const
	{
	return filter_2pole( *this, cutoff, damping, FLANHIP_FILTER2_NOTCH, order, "filter_2pole_notch" );
	}

// :646-654: the gain through sample_function_over_domain, at f * ( 1.0f / sr ), but cutoff and damping at frame_to_time( f ) = f / sr -- not
// always the same float.  gain / 2.0f and -gain are exact and are the device's
static Audio filter_2pole_shelf( const Audio & me, const Function<Second, Frequency> & cutoff, const Function<Second, float> & damping,
	const Function<Second, Decibel> & gain, int kind, uint16_t order, const char * who )
	{
	if( me.is_null() || !me.device_data() ) return Audio::create_null();     // :716
	const Frame n = me.get_num_frames();
	auto at = [&me]( int x ){ return me.frame_to_time( fFrame( x ) ); };
	return filter2_cascade( me, upload_curve_at( cutoff, n, at ), upload_curve_at( damping, n, at ), upload_curve( gain, n, 1.0f / me.get_sample_rate() ),
		kind, order, who );
	}

Audio Audio::filter_2pole_lowshelf( const Function<Second, Frequency> & cutoff, const Function<Second, float> & damping,
	const Function<Second, Decibel> & gain, uint16_t order ) const
	{
	return filter_2pole_shelf( *this, cutoff, damping, gain, FLANHIP_FILTER2_LOWSHELF, order, "filter_2pole_lowshelf" );
	}

Audio Audio::filter_2pole_bandshelf( const Function<Second, Frequency> & cutoff, const Function<Second, float> & damping,
	const Function<Second, Decibel> & gain, uint16_t order ) const
	{
	return filter_2pole_shelf( *this, cutoff, damping, gain, FLANHIP_FILTER2_BANDSHELF, order, "filter_2pole_bandshelf" );
	}

Audio Audio::filter_2pole_highshelf( const Function<Second, Frequency> & cutoff, const Function<Second, float> & damping,
	const Function<Second, Decibel> & gain, uint16_t order ) const
	{
	return filter_2pole_shelf( *this, cutoff, damping, gain, FLANHIP_FILTER2_HIGHSHELF, order, "filter_2pole_highshelf" );
	}

// :452-454, :498: cutoff and gain through sample_function_over_domain; the tilt of gain or -gain and the final amp( gain / 2 ) are the device's
static Audio filter_1pole_shelf( const Audio & me, const Function<Second, Frequency> & cutoff, const Function<Second, Decibel> & gain, int kind,
	uint16_t order, const char * who )
	{
	if( me.is_null() || !me.device_data() ) return Audio::create_null();     // :496, :508
	const float step = 1.0f / me.get_sample_rate();
	return filter2_cascade( me, upload_curve( cutoff, me.get_num_frames(), step ), DeviceArg(), upload_curve( gain, me.get_num_frames(), step ),
		kind, order, who );
	}

Audio Audio::filter_1pole_lowshelf( const Function<Second, Frequency> & cutoff, const Function<Second, Decibel> & gain, uint16_t order ) const
	{
	return filter_1pole_shelf( *this, cutoff, gain, FLANHIP_FILTER2_1POLE_LOWSHELF, order, "filter_1pole_lowshelf" );
	}

Audio Audio::filter_1pole_highshelf( const Function<Second, Frequency> & cutoff, const Function<Second, Decibel> & gain, uint16_t order ) const
	{
	return filter_1pole_shelf( *this, cutoff, gain, FLANHIP_FILTER2_1POLE_HIGHSHELF, order, "filter_1pole_highshelf" );
	}

// :1008-1011: cutoff, feedback and wet_dry through sample_function_over_domain, at f * ( 1.0f / sr ); the clamp, the links and the recurrence
// are the device's
Audio Audio::filter_comb( const Function<Second, Frequency> & cutoff, const Function<Second, float> & feedback, const Function<Second, float> & wet_dry,
	bool invert ) const
	{
	if( is_null() || !device_data() ) return Audio::create_null();     // :995; without a device nothing is sampled
	const size_t ws_bytes = flanhip_filter_comb_workspace_bytes( get_num_channels(), get_num_frames() );
	if( ws_bytes == 0 ) return Audio::create_null();
	const float step = 1.0f / get_sample_rate();
	const DeviceArg c = upload_curve( cutoff, get_num_frames(), step ), k = upload_curve( feedback, get_num_frames(), step ),
		a = upload_curve( wet_dry, get_num_frames(), step );
	return audio_call( "filter_comb", get_format(), c.ok && k.ok && a.ok, ws_bytes, [&]( float * out, void * ws )
		{
		return flanhip_filter_comb_dev( device_data(), get_num_channels(), get_num_frames(), get_sample_rate(), c.ptr(), c.scalar, k.ptr(), k.scalar,
			a.ptr(), a.scalar, invert ? 1 : 0, out, ws, nullptr );
		} );
	}

// :813-815, :830-831, :912-915, :978: every parameter once per frame at f * ( 1.0f / sr ), as filter_comb samples; the clamp, the prewarp and the
// scan are the device's.  What the device form does not offer is refused here, before anything is sampled or uploaded
static Audio multinotch( const Audio & me, const char * name, int kind, uint16_t order, const Function<Second, Frequency> & cutoff,
	const Function<Second, float> * damping, const Function<Second, float> & feedback, bool invert, const Function<Second, float> & wet_dry, bool use_saturator )
	{
	if( me.is_null() ) return Audio::create_null();                    // :811, :910
	if( use_saturator )
		{
		std::cerr << "flan: " << name << ": use_saturator is not offered on the device (a Newton iteration per frame, not linear in the state)" << std::endl;
		return Audio::create_null();
		}
	const size_t ws_bytes = flanhip_multinotch_workspace_bytes( me.get_num_channels(), me.get_num_frames(), kind, order );
	if( ws_bytes == 0 )
		{
		std::cerr << "flan: " << name << " refused order " << order << " on " << me.get_num_channels() << " x " << me.get_num_frames()
		          << ": the order is 1 ... " << ( kind == FLANHIP_MULTINOTCH_1POLE ? 16 : 8 ) << std::endl;
		return Audio::create_null();
		}
	if( !me.device_data() ) return Audio::create_null();               // without a device nothing is sampled
	const Frame n = me.get_num_frames();
	const float step = 1.0f / me.get_sample_rate();
	const DeviceArg c = upload_curve( cutoff, n, step ), R = damping ? upload_curve( *damping, n, step ) : DeviceArg(),
		k = upload_curve( feedback, n, step ), a = upload_curve( wet_dry, n, step );
	return audio_call( name, me.get_format(), c.ok && R.ok && k.ok && a.ok, ws_bytes, [&]( float * out, void * ws )
		{
		return flanhip_multinotch_dev( me.device_data(), me.get_num_channels(), n, me.get_sample_rate(), c.ptr(), c.scalar, R.ptr(), R.scalar,
			k.ptr(), k.scalar, a.ptr(), a.scalar, kind, order, invert ? 1 : 0, out, ws, nullptr );
		} );
	}

Audio Audio::filter_1pole_multinotch( uint16_t order, const Function<Second, Frequency> & cutoff, const Function<Second, float> & feedback, bool invert,
	const Function<Second, float> & wet_dry, bool use_saturator ) const
	{
	return multinotch( *this, "filter_1pole_multinotch", FLANHIP_MULTINOTCH_1POLE, order, cutoff, nullptr, feedback, invert, wet_dry, use_saturator );
	}

Audio Audio::filter_2pole_multinotch( uint16_t order, const Function<Second, Frequency> & cutoff, const Function<Second, float> & damping,
	const Function<Second, float> & feedback, bool invert, const Function<Second, float> & wet_dry, bool use_saturator ) const
	{
	return multinotch( *this, "filter_2pole_multinotch", FLANHIP_MULTINOTCH_2POLE, order, cutoff, &damping, feedback, invert, wet_dry, use_saturator );
	}

// :1168: the modulator through sample_function_over_domain, at f * ( 1.0f / sr ); the network and the product are the device's
Audio Audio::halfband_modulate( const Function<Second, std::complex<float>> & modulator ) const
	{
	if( is_null() || !device_data() ) return Audio::create_null();     // :1166; without a device nothing is sampled
	DeviceArg re, im;
	if( modulator.is_constant() ) { re.scalar = modulator.get_constant().real(); im.scalar = modulator.get_constant().imag(); }
	else
		{
		const Frame n = get_num_frames();
		const float step = 1.0f / get_sample_rate();
		detail::StagingVector<float> res( static_cast<size_t>( n ) ), ims( static_cast<size_t>( n ) );
		detail::for_each_index( 0, n, modulator.get_execution_policy(), [&]( int x )
			{
			const std::complex<float> m = modulator( Second( x * step ) );
			res[size_t( x )] = m.real(); ims[size_t( x )] = m.imag();
			} );
		re = upload_values( res ); im = upload_values( ims );
		}
	return halfband_modulated( *this, re, im, nullptr, "halfband_modulate" );
	}

Audio Audio::shift_frequency( const Function<Second, Frequency> & shift, const Frequency low_cutoff ) const
	{
	if( is_null() || !device_data() ) return Audio::create_null();     // :1193; without a device nothing is sampled
	const Frame n = get_num_frames();
	const float sr = get_sample_rate(), step = 1.0f / sr;
	const Frequency high_cutoff = sr / 2 - 1000;                       // :1195
	// :1203, :1211, :1223: the frame a time sampled at f * ( 1.0f / sr ) is read back as, in fp32; n reads the last frame
	auto frame_of = [&]( Frame f ){ return std::clamp( Frame( std::round( time_to_frame( Second( f * step ) ) ) ), Frame( 0 ), n - 1 ); };
	// :1218-1219: shift * pi2 / sr summed one frame after the other from 0.0f, exclusive
	detail::StagingVector<float> phase( static_cast<size_t>( n ) );
	DeviceArg lp, hp;
	if( shift.is_constant() )
		{
		const Frequency s = shift.get_constant();
		lp.scalar = s > 0 ? high_cutoff - s : high_cutoff;             // :1204-1207
		hp.scalar = s < 0 ? low_cutoff - s : low_cutoff;               // :1212-1215
		const float inc = s * pi2 / sr;
		float sum = 0.0f;
		for( Frame f = 0; f < n; ++f ) { phase[size_t( f )] = sum; sum = sum + inc; }
		}
	else
		{
		detail::StagingVector<float> sampled( static_cast<size_t>( n ) ), lps( static_cast<size_t>( n ) ), hps( static_cast<size_t>( n ) );
		detail::for_each_index( 0, n, shift.get_execution_policy(), [&]( int x ){ sampled[size_t( x )] = shift( Second( x * step ) ); } );
		for( Frame f = 0; f < n; ++f )
			{
			const Frequency s = sampled[size_t( frame_of( f ) )];
			lps[size_t( f )] = s > 0 ? high_cutoff - s : high_cutoff;
			hps[size_t( f )] = s < 0 ? low_cutoff - s : low_cutoff;
			}
		float sum = 0.0f;
		for( Frame f = 0; f < n; ++f ) { phase[size_t( f )] = sum; sum = sum + sampled[size_t( f )] * pi2 / sr; }
		lp = upload_values( lps ); hp = upload_values( hps );
		}
	detail::StagingVector<float> read( static_cast<size_t>( n ) );     // :1223-1225: the modulator reads the phase through the same round trip
	for( Frame f = 0; f < n; ++f ) read[size_t( f )] = phase[size_t( frame_of( f ) )];
	const DeviceArg d_phase = upload_values( read );
	const Audio antialiased = filter_cascade( filter_cascade( *this, lp, FLANHIP_FILTER_BUTTERWORTH_LOW, 8, "shift_frequency" ), hp,
		FLANHIP_FILTER_BUTTERWORTH_HIGH, 8, "shift_frequency" );
	if( antialiased.is_null() ) return Audio::create_null();
	return halfband_modulated( antialiased, DeviceArg(), DeviceArg(), &d_phase, "shift_frequency" );
	}

Audio Audio::halfband_multiply( const Audio & modulator ) const
	{
	if( is_null() || modulator.is_null() || !device_data() ) return Audio::create_null();     // :1233; the reference dereferences a null modulator
	auto bandpass_antialias = []( const Audio & a )                    // :1235-1240
		{
		const DeviceArg low( 30.0f ), high( a.get_sample_rate() / 2 - 2000 );
		return filter_cascade( filter_cascade( a, high, FLANHIP_FILTER_BUTTERWORTH_LOW, 8, "halfband_multiply" ), low,
			FLANHIP_FILTER_BUTTERWORTH_HIGH, 8, "halfband_multiply" );
		};
	const Audio a = bandpass_antialias( *this ), b = bandpass_antialias( modulator );
	if( a.is_null() || b.is_null() ) return Audio::create_null();
	AudioBuffer::Format f = get_format();                              // :1245-1247
	f.num_channels = std::min( get_num_channels(), modulator.get_num_channels() );
	f.num_frames = std::min( get_num_frames(), modulator.get_num_frames() );
	const size_t ws_bytes = flanhip_halfband_workspace_bytes( f.num_channels, f.num_frames );
	if( ws_bytes == 0 ) return Audio::create_null();
	const float * d_a = a.device_data(), * d_b = b.device_data();
	if( !d_a || !d_b ) return Audio::create_null();
	return audio_call( "halfband_multiply", f, true, ws_bytes, [&]( float * out, void * ws )
		{
		return flanhip_halfband_multiply_dev( d_a, a.get_num_channels(), a.get_num_frames(), a.get_sample_rate(), d_b, b.get_num_channels(), b.get_num_frames(), b.get_sample_rate(), out, ws, nullptr );
		} );
	}

// ---- channels (Audio/AudioConversions.cpp:58-104, Audio/AudioChannels.cpp) --------------------------------------------------------------
Audio Audio::convert_to_stereo() const
	{
	if( is_null() ) return Audio::create_null();                // AudioConversions.cpp:60
	if( get_num_channels() == 2 ) return copy();                // :78-79
	if( get_num_channels() != 1 )
		{
		std::cout << "I don't know how to convert that number of channels to stereo." << std::endl;     // :81
		return create_empty_with_frames( get_num_frames(), 2, get_sample_rate() );                      // the zero-initialised `out` of :64
		}
	const float * d_x = device_data();
	if( !d_x ) return Audio::create_null();
	AudioBuffer::Format f = get_format();
	f.num_channels = 2;
	return audio_call( "convert_to_stereo", f, true, detail::kNoWorkspace, [&]( float * out, void * )
		{ return flanhip_audio_to_stereo_dev( d_x, f.num_frames, out, nullptr ); } );
	}

Audio Audio::convert_to_mono() const
	{
	if( is_null() ) return Audio::create_null();                // :89
	const float * d_x = device_data();
	if( !d_x ) return Audio::create_null();
	AudioBuffer::Format f = get_format();
	f.num_channels = 1;
	return audio_call( "convert_to_mono", f, true, detail::kNoWorkspace, [&]( float * out, void * )
		{ return flanhip_audio_to_mono_dev( d_x, get_num_channels(), f.num_frames, out, nullptr ); } );
	}

std::vector<Audio> Audio::split_channels() const
	{
	std::vector<Audio> channels;                                // AudioChannels.cpp:16-28
	if( is_null() ) return channels;
	const float * d_x = device_data();
	AudioBuffer::Format f = get_format();
	f.num_channels = 1;
	DeviceCall call( "split_channels" );                        // a channel's block is handed out once its copy is launched; one wait for them all
	for( Channel channel = 0; channel < get_num_channels(); ++channel )
		{
		float * out = d_x ? call.output<float>( size_t( f.num_frames ) ) : nullptr;
		const bool ok = out && call.launch( flanhip_audio_copy_rows_dev( d_x + size_t( channel ) * size_t( f.num_frames ), f.num_frames, 1, f.num_frames,
			out, f.num_frames, f.num_frames, nullptr ) );
		channels.emplace_back( ok ? Audio( call.adopt<AudioBuffer>( f ) ) : Audio() );
		}
	if( d_x ) call.sync();
	return channels;
	}

Audio Audio::combine_channels( const std::vector<const Audio *> & channels_unmatched )
	{
	if( channels_unmatched.empty() ) return Audio::create_null();                  // :35
	for( const Audio * a : channels_unmatched ) if( !a || a->is_null() ) return Audio::create_null();
	// match_sample_rates_or_return_null (AudioCombination.cpp:17-35): unless all rates are the highest one, every input is resampled to it
	FrameRate max_sr = 0;
	bool all_match = true;
	for( const Audio * a : channels_unmatched ) max_sr = std::max( max_sr, a->get_sample_rate() );
	for( const Audio * a : channels_unmatched ) if( a->get_sample_rate() != max_sr ) all_match = false;
	std::vector<Audio> resampled;
	std::vector<const Audio *> channels = channels_unmatched;
	if( !all_match )
		{
		for( const Audio * a : channels_unmatched ) resampled.emplace_back( a->resample( max_sr ) );
		for( size_t i = 0; i < resampled.size(); ++i )
			{
			if( resampled[i].is_null() ) return Audio::create_null();
			channels[i] = &resampled[i];
			}
		}
	AudioBuffer::Format f;                                                         // :41-46
	f.sample_rate = channels[0]->get_sample_rate();
	f.num_channels = 0; f.num_frames = 0;
	for( const Audio * a : channels ) { f.num_channels += a->get_num_channels(); f.num_frames = std::max( f.num_frames, a->get_num_frames() ); }
	DeviceCall call( "combine_channels" );
	float * out = call.output<float>( size_t( f.num_channels ) * size_t( f.num_frames ) );
	if( !out ) return Audio::create_null();
	Channel current = 0;
	for( const Audio * a : channels )                                              // :50-59; what lies behind a shorter input is zero (:48)
		{
		const float * d_a = a->device_data();
		if( !d_a ) return Audio::create_null();
		if( !call.launch( flanhip_audio_copy_rows_dev( d_a, a->get_num_frames(), a->get_num_channels(), a->get_num_frames(),
				out + size_t( current ) * size_t( f.num_frames ), f.num_frames, f.num_frames, nullptr ) ) ) return Audio::create_null();
		current += a->get_num_channels();
		}
	return or_null( call.finish<AudioBuffer>( f ) );
	}

Audio Audio::combine_channels( const std::vector<Audio> & channels )
	{
	std::vector<const Audio *> ptrs;                                               // :64-67
	for( const Audio & a : channels ) ptrs.push_back( &a );
	return combine_channels( ptrs );
	}

// ---- spatial (Audio/AudioSpatial.cpp) -------------------------------------------------------------------------------------------------------
// pan_in_place's arithmetic (:27-38) over a stereo Audio into a fresh block; pan_amount through sample_function_over_domain, at f * ( 1.0f / sr )
static Audio panned( const Audio & stereo, const Function<Second, float> & pan_amount )
	{
	const float * d_x = stereo.device_data();
	if( !d_x ) return Audio();                                    // without a device nothing is sampled
	const DeviceArg p = upload_curve( pan_amount, stereo.get_num_frames(), 1.0f / stereo.get_sample_rate() );
	// (a failure is a plain null here: pan() says "Null Audio created", pan_in_place() keeps what it has)
	return detail::device_call<AudioBuffer, float>( "pan", stereo.get_format(), 2 * size_t( stereo.get_num_frames() ), p.ok, detail::kNoWorkspace,
		[&]( float * out, void * ){ return flanhip_audio_pan_dev( d_x, 2, stereo.get_num_frames(), p.ptr(), p.scalar, out, nullptr ); } );
	}

Audio Audio::pan( const Function<Second, float> & pan_amount ) const
	{
	if( is_null() ) return Audio::create_null();                // :11
	if( get_num_channels() != 1 && get_num_channels() != 2 ) return Audio::create_null();     // :13-14
	if( get_num_channels() == 2 ) { Audio out = panned( *this, pan_amount ); return out.is_null() ? Audio::create_null() : std::move( out ); }
	const Audio stereo = convert_to_stereo();                   // :16
	if( stereo.is_null() ) return Audio::create_null();
	Audio out = panned( stereo, pan_amount );
	return out.is_null() ? Audio::create_null() : std::move( out );
	}

Audio & Audio::pan_in_place( const Function<Second, float> & pan_amount )
	{
	if( is_null() ) { std::cout << "Null input" << std::endl; return *this; }      // :23
	if( get_num_channels() != 2 ) return *this;                 // :25
	Audio out = panned( *this, pan_amount );
	if( !out.is_null() ) *this = std::move( out );
	return *this;
	}

Audio Audio::widen( const Function<Second, float> & widen_amount ) const
	{
	return convert_to_mid_side().pan( widen_amount ).convert_to_left_right();      // :44
	}

Audio Audio::stereo_spatialize( const Function<Second, vec2> & position, Meter head_width, const Function<Second, float> & speed_limit ) const
	{
	if( get_num_channels() != 1 )
		{
		std::cout << "Audio::spacialize only operates on mono inputs." << std::endl;             // :231
		return Audio::create_null();
		}
	if( is_null() ) return Audio::create_null();
	const Frame n = get_num_frames();
	const Frame granularity_frames = 32;                                           // :137
	const float sr = get_sample_rate(), sound_mps = 343;                           // :7
	if( !position.is_constant() && n <= granularity_frames )
		{
		std::cout << "Audio::stereo_spatialize: a moving source needs more than 32 frames, the result would have none." << std::endl;
		return Audio();
		}
	const float * d_x = device_data();
	if( !d_x ) return Audio::create_null();                                        // without a device nothing is sampled
	// head_ild's low-pass (:128) is the same for both ears: once
	const Audio lowpassed = filter_cascade( *this, DeviceArg( 500.0f ), FLANHIP_FILTER_BUTTERWORTH_LOW, 1, "stereo_spatialize" );
	if( lowpassed.is_null() ) return Audio::create_null();
	DeviceCall call( "stereo_spatialize" );                                       // two launches: every `return` below the first waits for it
	float * shaped = static_cast<float*>( call.scratch( sizeof( float ) * 2 * size_t( n ) ) );
	if( !shaped ) return Audio::create_null();
	const vec2d ear_position[2] = { vec2d( 0, 1 * head_width / 2.0f ), vec2d( 0, -1 * head_width / 2.0f ) };    // :261, the left ear first
	AudioBuffer::Format f = get_format();
	f.num_channels = 2;
	int64_t out_frames[2] = { 0, 0 };

	if( position.is_constant() )
		{
		// :139-153: both ears a pure delay.  head_ild and falloff see one position (:263, the transform of a constant)
		const vec2d p = vec2d( position.get_constant() );                          // :235
		float delays[2];
		for( int e = 0; e < 2; ++e )
			{
			const Meter dist = ( p - ear_position[e] ).mag();                      // :141-142
			delays[e] = time_to_frame( dist / sound_mps );                         // :143
			out_frames[e] = Frame( n + delays[e] );                                // :148
			}
		f.num_frames = Frame( std::max( out_frames[0], out_frames[1] ) );
		if( !call.launch( flanhip_spatial_ear_dev( d_x, lowpassed.device_data(), 1, n, sr, nullptr, p.x(), p.y(), head_width, FLANHIP_SPATIAL_BOTH,
				shaped, nullptr ) ) ) return Audio::create_null();
		float * out = call.output<float>( 2 * size_t( f.num_frames ) );
		if( !out ) return Audio::create_null();
		call.launch( flanhip_spatial_delay_dev( shaped, 2, n, delays, out_frames, f.num_frames, out, nullptr ) );
		return or_null( call.finish<AudioBuffer>( f ) );                           // combine_channels( l, r ) (:280): the longer ear's length
		}

	// :235: the position once per frame, as doubles
	detail::StagingVector<double> ps( 2 * size_t( n ) );
	{
	const float step = 1.0f / sr;
	detail::for_each_index( 0, n, position.get_execution_policy(), [&]( int x )
		{
		const vec2 v = position( Second( x * step ) );
		ps[2 * size_t( x )] = v.x(); ps[2 * size_t( x ) + 1] = v.y();
		} );
	}
	// :238-257: the speed limiter.  It stays on the host: frame f needs the LIMITED frame f - 1, the step is not linear in it (a division by the
	// movement's length), so no scan composes it; it is one pass over 16 n bytes
	{
	const float epsilon = 1;
	const auto limit = speed_limit.sample( 0, n, 1.0f / sr );                      // :246
	for( Frame frame = 1; frame < n; ++frame )
		{
		const vec2d previous( ps[2 * size_t( frame ) - 2], ps[2 * size_t( frame ) - 1] );
		const vec2d movement = vec2d( ps[2 * size_t( frame )], ps[2 * size_t( frame ) + 1] ) - previous;
		const Meter mag = movement.mag();
		const float limit_here = limit.is_constant() ? limit.get_constant() : limit.get_vector()[size_t( frame )];
		const float speed_limit_c = std::clamp( limit_here, 0.0f, sound_mps - epsilon ) / sr;        // :253
		if( mag > speed_limit_c )
			{
			const vec2d limited = previous + movement / mag * speed_limit_c;       // :255
			ps[2 * size_t( frame )] = limited.x(); ps[2 * size_t( frame ) + 1] = limited.y();
			}
		}
	}
	// :159-186 per ear: the distances at frames 0, 32, ... give the stretches and the output length
	const int64_t count = ( int64_t( n ) + granularity_frames - 1 ) / granularity_frames;
	const size_t chunks = size_t( count );
	std::vector<double> distances( chunks ), stretches( 2 * chunks );
	for( int e = 0; e < 2; ++e )
		{
		for( int64_t k = 0; k < count; ++k )
			distances[size_t( k )] = ( vec2d( ps[2 * size_t( k ) * granularity_frames], ps[2 * size_t( k ) * granularity_frames + 1] ) - ear_position[e] ).mag();
		out_frames[e] = flanhip_spatial_itd_out_frames( n, sr, distances.data(), count, stretches.data() + size_t( e ) * size_t( count ) );
		if( out_frames[e] < 0 ) { detail::report( int( out_frames[e] ), "stereo_spatialize" ); return Audio::create_null(); }
		}
	f.num_frames = Frame( std::min<int64_t>( std::max( out_frames[0], out_frames[1] ), std::numeric_limits<Frame>::max() ) );
	const size_t ws_bytes = flanhip_spatial_itd_workspace_bytes( 2, n, sr, stretches.data(), count );
	if( f.num_frames <= 0 || ws_bytes == 0 )
		{
		std::cerr << "flan: stereo_spatialize refused " << n << " frames: ";
		if( ws_bytes == 0 ) std::cerr << flanhip_last_error(); else std::cerr << "no output frames";
		std::cerr << std::endl;
		return Audio::create_null();
		}
	double * d_ps = static_cast<double*>( call.scratch( sizeof( double ) * ps.size() ) );
	float * out = call.output<float>( 2 * size_t( f.num_frames ) );
	void * ws = call.workspace( ws_bytes );
	if( !call.ok() ) return Audio::create_null();
	if( !detail::upload_from_host( d_ps, ps.data(), sizeof( double ) * ps.size() ) )
		{
		std::cerr << "flan: upload of the sampled positions failed: " << flanhip_last_error() << std::endl;
		return Audio::create_null();
		}
	if( !call.launch( flanhip_spatial_ear_dev( d_x, lowpassed.device_data(), 1, n, sr, d_ps, 0.0, 0.0, head_width, FLANHIP_SPATIAL_BOTH, shaped, nullptr ) ) )
		return Audio::create_null();
	call.launch( flanhip_spatial_itd_dev( shaped, 2, n, sr, stretches.data(), count, out_frames, f.num_frames, out, ws, nullptr ) );
	return or_null( call.finish<AudioBuffer>( f ) );                               // combine_channels( l, r ) (:280): the longer ear's length
	}

// ---- information (Audio/AudioInformation.cpp) -----------------------------------------------------------------------------------------------
// `count` floats that launch( d_out ) leaves on the device, brought to the host; false (and `who` on std::cerr) if anything failed
template<typename Launch>
static bool wavelengths_call( const char * who, std::vector<float> & out, size_t ws_bytes, Launch launch )
	{
	DeviceCall call( who );
	float * d_out = call.output<float>( out.size() );
	void * ws = ws_bytes == detail::kNoWorkspace ? nullptr : call.workspace( ws_bytes );
	if( !call.ok() || !call.launch( launch( d_out, ws ) ) || !call.sync() ) return false;
	if( detail::download_to_host( out.data(), d_out, sizeof( float ) * out.size() ) ) return true;
	std::cerr << "flan: " << who << ": download failed: " << flanhip_last_error() << std::endl;
	return false;
	}

float Audio::get_local_wavelength( Channel channel, Frame start, Frame window_size, float absolute_cutoff, Frame minimum_wavelength ) const
	{
	if( is_null() ) return 0;                                                      // :140
	if( channel < 0 || channel >= get_num_channels() || start < 0 || window_size < 1 || start > get_num_frames() - window_size )
		{
		std::cerr << "flan: get_local_wavelength: the window lies outside the signal" << std::endl;      // the reference reads past its buffer
		return 0;
		}
	const float * d_x = device_data();
	if( !d_x ) return 0;
	std::vector<float> out( 1 );
	const float * d_window = d_x + size_t( channel ) * size_t( get_num_frames() ) + size_t( start );     // :143 get_sample_pointer( channel, start )
	if( !wavelengths_call( "get_local_wavelength", out, detail::kNoWorkspace, [&]( float * d_out, void * )
		{ return flanhip_audio_local_wavelength_dev( d_window, window_size, absolute_cutoff, minimum_wavelength, d_out, nullptr ); } ) ) return 0;
	return out[0];
	}

std::vector<fFrame> Audio::get_local_wavelengths( Channel channel, Frame start, Frame end, Frame window_size, Frame hop, float absolute_cutoff,
	Frame minimum_wavelength, flan_CANCEL_ARG_CPP ) const
	{
	if( is_null() ) return std::vector<float>();                                   // :178
	if( canceller ) return std::vector<float>();                                   // :185
	const Frame n = get_num_frames();
	const int64_t count = flanhip_audio_local_wavelengths_count( n, start, end, window_size, hop );      // :180-187
	const size_t ws_bytes = flanhip_audio_local_wavelengths_workspace_bytes( n, start, end, window_size, hop );
	if( channel < 0 || channel >= get_num_channels() || count < 0 || ws_bytes == 0 )
		{
		std::cerr << "flan: get_local_wavelengths: a channel, range, hop or window the device does not take (windows go up to 16384 frames)" << std::endl;
		return std::vector<float>();
		}
	if( count == 0 ) return std::vector<float>();                                  // :188
	const float * d_x = device_data();
	if( !d_x ) return std::vector<float>();
	std::vector<fFrame> out( static_cast<size_t>( count ) );
	if( !wavelengths_call( "get_local_wavelengths", out, ws_bytes, [&]( float * d_out, void * ws )
		{
		return flanhip_audio_local_wavelengths_dev( d_x + size_t( channel ) * size_t( n ), n, start, end, window_size, hop, absolute_cutoff, minimum_wavelength,
			d_out, ws, nullptr );
		} ) ) return std::vector<float>();
	if( canceller ) return std::vector<float>();
	flanhip_wavelength_continuity( out.data(), count, get_sample_rate(), hop );    // :190-226
	return out;
	}

float Audio::get_average_wavelength( Channel channel, float min_active_ratio, float max_length_sigma, Frame start, Frame end, Frame window_size, Frame hop,
	flan_CANCEL_ARG_CPP ) const
	{
	if( is_null() ) return 0;                                                      // :241
	return get_average_wavelength( get_local_wavelengths( channel, start, end, window_size, hop, 0.2f, 10, canceller ), min_active_ratio, max_length_sigma );
	}

float Audio::get_average_wavelength( const std::vector<float> & locals, float min_active_ratio, float max_length_sigma ) const
	{
	if( is_null() ) return 0;                                                      // :251
	float mean = 0;
	flanhip_average_wavelength( locals.data(), int64_t( locals.size() ), min_active_ratio, max_length_sigma, &mean );
	return mean;
	}

Frequency Audio::get_local_frequency( Channel channel, Frame start, Frame window_size, flan_CANCEL_ARG_CPP ) const
	{
	(void) canceller;
	const fFrame wavelength = get_local_wavelength( channel, start, window_size, 0.2f, 10 );     // :269
	return get_sample_rate() / wavelength;                                         // a 0 gives infinity, as in the reference
	}

std::vector<Frequency> Audio::get_local_frequencies( Channel channel, Frame start, Frame end, Frame window_size, Frame hop, flan_CANCEL_ARG_CPP ) const
	{
	std::vector<fFrame> wavelengths = get_local_wavelengths( channel, start, end, window_size, hop, 0.2f, 10, canceller );      // :298
	for( float & w : wavelengths ) if( w != 0 ) w = get_sample_rate() / w;         // :299-303
	return wavelengths;
	}

Function<Second, Amplitude> Audio::get_frequency_envelope() const
	{
	if( is_null() ) return 0.0f;
	const int hop_size = 128;                                                      // :391-392
	std::vector<Frequency> frequencies = convert_to_mono().get_local_frequencies( 0, 0, -1, 2048, hop_size );
	if( frequencies.empty() ) return 0.0f;                                         // the reference's lambda would read an empty vector
	return [frequencies = std::move( frequencies ), sample_rate = get_sample_rate(), hop_size]( Second t )      // :394-406
		{
		const float x = t * sample_rate / hop_size;
		if( 0 <= x && x < frequencies.size() - 1 )
			{
			const Frame x1 = std::floor( x );
			const float y1 = frequencies[x1];
			const float y2 = frequencies[x1 + 1];
			const float m = ( y2 - y1 ) / 1;
			return y1 + m * ( x - x1 );
			}
		else return 0.0f;
		};
	}

// ---- cutting, mixing and granular synthesis (Audio/AudioCombination.cpp, Audio/AudioTemporal.cpp:190-234, Audio/AudioSynthesis.cpp) ----------------
namespace {

// A table of events as the device takes it: every src a device address, the amplitudes that are not constants in one pool
struct EventTable
	{
	std::vector<flanhip_grain_event> events;
	std::vector<float> gains;
	};

flanhip_grain_event plain_event()
	{
	flanhip_grain_event e = {};
	e.gain_offset = -1;
	e.gain = 1.0f;
	return e;
	}

// `a` as the source of an event; false if its samples cannot be had on the device
bool point_at( const Audio & a, flanhip_grain_event & e )
	{
	const float * d = a.device_data();
	if( !d ) return false;
	e.src = uint64_t( reinterpret_cast<uintptr_t>( d ) );
	e.ch_stride = a.get_num_frames(); e.src_frames = a.get_num_frames();
	e.channels = a.get_num_channels();
	return true;
	}

// `a` from its first frame on, or nothing if a is a null Audio
bool whole_event( const Audio & a, flanhip_grain_event & e )
	{
	if( a.is_null() ) return true;
	e.n = a.get_num_frames();
	return point_at( a, e );
	}

// The sink: the table's length (AudioCombination.cpp:146-150), or the caller's, and plan on the host, then one launch.  Nothing to hear -- no frames, or no event
// with any -- is the reference's null Audio
Audio mix_events( const char * who, const EventTable & table, Channel channels, FrameRate sample_rate, int64_t out_frames = 0 )
	{
	const int64_t count = int64_t( table.events.size() );
	bool live = false;
	for( const flanhip_grain_event & e : table.events ) live = live || ( e.n > 0 && e.channels > 0 );
	int64_t frames = std::max<int64_t>( out_frames, 0 );                           // 0: the table's own length; else the caller's (events are clipped to it)
	if( !live || channels < 1 || flanhip_grains_plan( table.events.data(), count, &frames, nullptr, nullptr, 0 ) != FLANHIP_OK ) return Audio::create_null();
	if( frames < 1 || frames > INT_MAX )
		{
		std::cerr << "flan: " << who << ": an output of " << frames << " frames" << std::endl;
		return Audio::create_null();
		}
	const int64_t tile = flanhip_grains_tile_frames(), tiles = ( frames + tile - 1 ) / tile;
	std::vector<int32_t> first( static_cast<size_t>( tiles ) ), last( static_cast<size_t>( tiles ) );
	if( flanhip_grains_plan( table.events.data(), count, &frames, first.data(), last.data(), tiles ) != FLANHIP_OK ) return Audio::create_null();
	const DeviceArg gains = table.gains.empty() ? DeviceArg( 0.0f ) : DeviceArg::from_host( table.gains.data(), sizeof( float ) * table.gains.size(), "sampled amplitudes" );
	AudioBuffer::Format f;
	f.num_channels = channels; f.num_frames = Frame( frames ); f.sample_rate = sample_rate;
	return audio_call( who, f, gains.ok, flanhip_grains_workspace_bytes( count, frames ), [&]( float * out, void * ws )
		{
		return flanhip_grains_mix_dev( table.events.data(), count, first.data(), last.data(), tiles, gains.ptr(), int64_t( table.gains.size() ), nullptr, 0,
			channels, frames, sample_rate, out, ws, nullptr );
		} );
	}

// a time as a frame by truncation (the reference's Frame( time_to_frame( t ) )); false for what no Frame holds
bool frame_of( Second t, FrameRate sample_rate, Frame & frame )
	{
	const float f = t * sample_rate;
	if( !( f > -2147483648.0f && f < 2147483648.0f ) ) return false;
	frame = Frame( f );
	return true;
	}

// Audio::mix (AudioCombination.cpp:102-170).  amplitude i is functions[i] where there are functions, else constants[i]; 1 behind the list's end
Audio mix_core( std::vector<const Audio *> ins_unmatched, std::vector<Second> start_times, const std::vector<const Function<Second, Amplitude> *> * functions,
	const std::vector<Amplitude> * constants )
	{
	if( ins_unmatched.empty() ) return Audio::create_null();                       // :109
	for( const Audio * a : ins_unmatched ) if( !a ) return Audio::create_null();
	const size_t num_amplitudes = functions ? functions->size() : constants ? constants->size() : 0;
	if( functions ) for( const auto * fn : *functions ) if( !fn ) return Audio::create_null();
	const size_t num_sources = std::max( { ins_unmatched.size(), start_times.size(), num_amplitudes } );      // :111

	// match_sample_rates_or_return_null (:17-35), over the inputs that are not null Audios
	FrameRate max_sr = 0;
	bool all_match = true;
	for( const Audio * a : ins_unmatched ) if( !a->is_null() ) max_sr = std::max( max_sr, a->get_sample_rate() );
	if( max_sr <= 0 ) return Audio::create_null();                                 // nothing but null Audios
	for( const Audio * a : ins_unmatched ) if( !a->is_null() && a->get_sample_rate() != max_sr ) all_match = false;
	std::vector<Audio> resampled;
	std::vector<const Audio *> ins = ins_unmatched;
	if( !all_match )
		{
		for( const Audio * a : ins_unmatched ) resampled.emplace_back( a->is_null() ? Audio() : a->resample( max_sr ) );
		for( size_t i = 0; i < resampled.size(); ++i )
			{
			if( resampled[i].is_null() && !ins_unmatched[i]->is_null() ) return Audio::create_null();
			ins[i] = &resampled[i];
			}
		}
	const size_t initial_num_ins = ins.size();                                     // :117-123
	for( size_t i = ins.size(); i < num_sources; ++i ) ins.push_back( ins[i % initial_num_ins] );
	start_times.resize( num_sources, 0 );

	EventTable table;
	table.events.resize( num_sources, plain_event() );
	Channel channels = 0;
	const float step = 1.0f / max_sr;                                              // frame_to_time( 1 ) (:138)
	for( size_t i = 0; i < num_sources; ++i )
		{
		flanhip_grain_event & e = table.events[i];
		Frame start = 0;
		if( !frame_of( start_times[i], max_sr, start ) )                           // :127-129
			{
			std::cerr << "flan: mix: a start time no frame holds" << std::endl;
			return Audio::create_null();
			}
		e.o = start;
		if( !whole_event( *ins[i], e ) ) return Audio::create_null();
		channels = std::max( channels, Channel( e.channels ) );                    // :144
		if( i >= num_amplitudes ) continue;                                        // :135-137: the constant 1
		if( constants ) { e.gain = ( *constants )[i]; continue; }
		const Function<Second, Amplitude> & fn = *( *functions )[i];
		if( fn.is_constant() ) { e.gain = fn.get_constant(); continue; }
		if( e.n == 0 ) continue;
		e.gain_offset = int64_t( table.gains.size() );                             // :138: sampled over [start, start + frames) at global time
		table.gains.resize( table.gains.size() + size_t( e.n ) );
		float * g = table.gains.data() + e.gain_offset;
		detail::for_each_index( 0, e.n, fn.get_execution_policy(), [&]( int x ){ g[x] = fn( Second( ( start + x ) * step ) ); } );
		}
	return mix_events( "mix", table, channels, max_sr );
	}

// integrate_event_rate (AudioSynthesis.cpp:310-374): the event frames; both Functions sampled over the frames of `length` at f * ( 1.0f / sample_rate )
std::vector<int64_t> event_frames( Second length, const Function<Second, float> & events_per_second, const Function<Second, float> & scatter, FrameRate sample_rate )
	{
	Frame length_frames = 0;
	if( !( sample_rate > 0 ) || !frame_of( length, sample_rate, length_frames ) || length_frames < 1 ) return {};      // :317
	const auto rate = events_per_second.sample( 0, length_frames, 1.0f / sample_rate );       // :319-323
	const auto scat = scatter.sample( 0, length_frames, 1.0f / sample_rate );
	static std::atomic<uint64_t> calls( 0 );
	const uint64_t seed = uint64_t( std::time( nullptr ) ) * 0x100000001B3ull + calls.fetch_add( 1 );      // :342: the clock
	std::vector<int64_t> frames( static_cast<size_t>( length_frames ) );
	int64_t count = 0;
	if( flanhip_grains_events( length_frames, sample_rate, rate.is_constant() ? nullptr : rate.get_vector().data(), rate.is_constant() ? rate.get_constant() : 0.0f,
			scat.is_constant() ? nullptr : scat.get_vector().data(), scat.is_constant() ? scat.get_constant() : 0.0f, seed, frames.data(), length_frames, &count ) != FLANHIP_OK )
		{
		std::cerr << "flan: the event rate was refused: " << flanhip_last_error() << std::endl;
		return {};
		}
	frames.resize( static_cast<size_t>( count ) );
	return frames;
	}

std::vector<Second> event_times_of( const std::vector<int64_t> & frames, FrameRate sample_rate )
	{
	std::vector<Second> times( frames.size() );
	for( size_t i = 0; i < frames.size(); ++i ) times[i] = Frame( frames[i] ) / sample_rate;       // :371
	return times;
	}

std::vector<const Audio *> pointers_to( const std::vector<Audio> & v )
	{
	std::vector<const Audio *> p;
	for( const Audio & a : v ) p.push_back( &a );
	return p;
	}

// WindowFunctions.cpp:10-13; the unqualified cos is the double one
float hann_window( float x ) { return float( 0.5f * ( 1.0f - std::cos( double( 2.0f * pi * x ) ) ) ); }

// Audio::granulate (AudioSynthesis.cpp:572-609) over curves already sampled for the frames of `length` (a constant, or one value per frame);
// hann: psola's window, in the kernel on the fused path and behind the mod on the general one (:621-627)
struct SampledCurve
	{
	const std::vector<float> * values; float constant;
	float at( Frame f ) const { return values ? ( *values )[size_t( f )] : constant; }
	};

Audio granulate_sampled( const Audio & me, const std::vector<int64_t> & frames, Frame sampled_frames, const SampledCurve & selection, const SampledCurve & grain_length,
	const SampledCurve & fade, const AudioMod & mod, bool hann )
	{
	const FrameRate sr = me.get_sample_rate();
	const size_t count = frames.size();
	if( count == 0 ) return Audio::create_null();                                  // mix of no inputs (AudioCombination.cpp:109)
	const std::vector<Second> times = event_times_of( frames, sr );
	std::vector<float> start( count ), end( count ), fades( count );
	EventTable table;
	table.events.resize( count, plain_event() );
	for( size_t i = 0; i < count; ++i )
		{
		Frame at = 0;                                                              // :590-592: the curves at time_to_frame( t )
		if( !frame_of( times[i], sr, at ) || at < 0 || at >= sampled_frames ) { start[i] = 0; end[i] = 0; fades[i] = 0; at = 0; }       // (cannot happen: at <= the event's frame)
		else { start[i] = selection.at( at ); end[i] = start[i] + grain_length.at( at ); fades[i] = fade.at( at ); }      // :593
		table.events[i].o = at;                                                    // mix's time_to_frame( t ) (AudioCombination.cpp:127-129)
		}
	if( flanhip_grains_cut( me.get_num_frames(), sr, int64_t( count ), start.data(), end.data(), fades.data(), fades.data(), table.events.data() ) != FLANHIP_OK )
		{
		std::cerr << "flan: granulate: " << flanhip_last_error() << std::endl;
		return Audio::create_null();
		}
	for( flanhip_grain_event & e : table.events ) if( !point_at( me, e ) ) return Audio::create_null();
	if( mod.is_null() )                                                            // the fused path: every grain cut, faded and windowed in flight
		{
		if( hann ) for( flanhip_grain_event & e : table.events ) e.flags = FLANHIP_GRAIN_HANN;
		return mix_events( "granulate", table, me.get_num_channels(), sr );
		}
	// the general path: a grain is one event mixed alone (which is cut_frames with its fades), then the mod's, then one event of the final mix
	std::vector<Audio> grains;
	grains.reserve( count );
	for( size_t i = 0; i < count; ++i )
		{
		flanhip_grain_event e = table.events[i];
		e.o = 0;
		EventTable one;
		one.events.push_back( e );
		Audio grain = e.n > 0 ? mix_events( "granulate", one, me.get_num_channels(), sr ) : Audio();
		mod( grain, times[i] );                                                    // :604-605
		if( hann && !grain.is_null() )
			grain.modify_volume_in_place( Function<Second, float>( [length = grain.get_length()]( Second t ){ return hann_window( t / length ); } ) );   // :626
		grains.emplace_back( std::move( grain ) );
		}
	return mix_core( pointers_to( grains ), times, nullptr, nullptr );             // synthesize_grains' Audio::mix( grains, event_times ) (:397)
	}

// a Function of time sampled over [0, frames) at f * step as a SampledCurve over `storage`
SampledCurve sampled_curve( const Function<Second, float> & fn, Frame frames, float step, std::vector<float> & storage )
	{
	if( fn.is_constant() ) return SampledCurve{ nullptr, fn.get_constant() };
	storage.resize( size_t( std::max( frames, 0 ) ) );
	detail::for_each_index( 0, frames, fn.get_execution_policy(), [&]( int x ){ storage[size_t( x )] = fn( Second( x * step ) ); } );
	return SampledCurve{ &storage, 0.0f };
	}

} // namespace

Audio Audio::cut( Second start_time, Second end_time, Second start_fade, Second end_fade ) const
	{
	if( is_null() ) return Audio::create_null();                                   // AudioTemporal.cpp:197
	EventTable table;
	table.events.push_back( plain_event() );
	if( flanhip_grains_cut( get_num_frames(), get_sample_rate(), 1, &start_time, &end_time, &start_fade, &end_fade, table.events.data() ) != FLANHIP_OK
		|| table.events[0].n <= 0 || !point_at( *this, table.events[0] ) ) return Audio::create_null();
	return mix_events( "cut", table, get_num_channels(), get_sample_rate() );
	}

Audio Audio::cut_frames( Frame start, Frame end, Frame start_fade, Frame end_fade ) const
	{
	if( is_null() ) return Audio::create_null();                                   // :214
	EventTable table;
	table.events.push_back( plain_event() );
	if( flanhip_grains_cut_frames( get_num_frames(), 1, &start, &end, &start_fade, &end_fade, table.events.data() ) != FLANHIP_OK
		|| table.events[0].n <= 0 || !point_at( *this, table.events[0] ) ) return Audio::create_null();
	return mix_events( "cut_frames", table, get_num_channels(), get_sample_rate() );
	}

Audio Audio::mix( std::vector<const Audio *> ins, std::vector<Second> start_times, std::vector<Amplitude> amplitudes )
	{
	return mix_core( std::move( ins ), std::move( start_times ), nullptr, &amplitudes );        // AudioCombination.cpp:78-91: constants stay scalars
	}

Audio Audio::mix( const std::vector<Audio> & ins, std::vector<Second> start_times, std::vector<Amplitude> amplitudes )
	{
	return mix( pointers_to( ins ), std::move( start_times ), std::move( amplitudes ) );        // :93-100
	}

Audio Audio::mix( std::vector<const Audio *> ins, std::vector<Second> start_times, const std::vector<const Function<Second, Amplitude> *> & amplitudes )
	{
	return mix_core( std::move( ins ), std::move( start_times ), &amplitudes, nullptr );        // :102-170
	}

Audio Audio::mix( const std::vector<Audio> & ins, const std::vector<Second> & start_times, const std::vector<Function<Second, Amplitude>> & amplitudes )
	{
	std::vector<const Function<Second, Amplitude> *> p;                            // :172-179
	for( const auto & fn : amplitudes ) p.push_back( &fn );
	return mix_core( pointers_to( ins ), start_times, &p, nullptr );
	}

Audio Audio::join( const std::vector<const Audio *> & ins, const std::vector<Second> & offsets )
	{
	if( ins.empty() || offsets.size() != ins.size() + 1 ) return Audio::create_null();         // :210
	for( const Audio * a : ins ) if( !a ) return Audio::create_null();
	std::vector<Second> start_times = { 0 };                                       // :212-218
	for( size_t i = 0; i + 1 < ins.size(); ++i )
		start_times.push_back( start_times.back() + ins[i]->get_length() + offsets[i + 1] );
	return mix( ins, start_times, std::vector<Amplitude>() );
	}

Audio Audio::join( const std::vector<const Audio *> & ins, Second offset )
	{
	return join( ins, std::vector<Second>( ins.size() + 1, offset ) );             // :223-229
	}

Audio Audio::join( const std::vector<Audio> & ins, Second offset )
	{
	return join( pointers_to( ins ), offset );                                     // :231-237
	}

Audio Audio::synthesize_grains( Second length, const Function<Second, float> & grains_per_second, const Function<Second, float> & time_scatter,
	const Function<Second, Audio> & grain_source, FrameRate sample_rate )
	{
	if( !( length > 0 ) ) return Audio::create_null();                             // AudioSynthesis.cpp:385
	const std::vector<Second> times = event_times_of( event_frames( length, grains_per_second, time_scatter, sample_rate ), sample_rate );
	std::vector<Audio> grains;                                                     // :390-395
	grains.reserve( times.size() );
	for( Second t : times ) grains.emplace_back( grain_source( t ) );
	return mix( grains, times );                                                   // :397
	}

Audio Audio::texture( Second length, const Function<Second, float> & grains_per_second, const Function<Second, float> & time_scatter, const AudioMod & mod,
	bool mod_feedback ) const
	{
	if( is_null() ) return Audio::create_null();                                   // :431
	if( !( length > 0 ) ) return Audio::create_null();                             // :412
	const std::vector<Second> times = event_times_of( event_frames( length, grains_per_second, time_scatter, get_sample_rate() ), get_sample_rate() );
	if( times.empty() ) return Audio::create_null();
	if( mod.is_null() )                                                            // synthesize_grains_repeat (:401-421): every event reads *this, gain 1
		return mix( std::vector<const Audio *>( times.size(), this ), times, std::vector<Amplitude>( times.size(), 1.0f ) );
	std::vector<Audio> modded;                                                     // :438-472
	modded.reserve( times.size() );
	for( size_t i = 0; i < times.size(); ++i )
		{
		Audio input = mod_feedback && i > 0 ? modded.back().copy() : copy();
		mod( input, mod_feedback && i == 0 ? 0 : times[i] );                       // :443: the first of a feedback chain is modded at time 0
		modded.emplace_back( std::move( input ) );
		}
	return mix( modded, times );
	}

Audio Audio::granulate( Second length, const Function<Second, float> & grains_per_second, const Function<Second, float> & time_scatter,
	const Function<Second, Second> & time_selection, const Function<Second, Second> & grain_length, const Function<Second, Second> & fade_time,
	const AudioMod & mod ) const
	{
	if( is_null() ) return Audio::create_null();                                   // :582
	Frame sampled_frames = 0;                                                      // :584-586
	if( !( length > 0 ) || !frame_of( length, get_sample_rate(), sampled_frames ) ) return Audio::create_null();      // synthesize_grains (:385)
	std::vector<float> s0, s1, s2;
	const float step = frame_to_time( 1 );
	const SampledCurve selection = sampled_curve( time_selection, sampled_frames, step, s0 ), lengths = sampled_curve( grain_length, sampled_frames, step, s1 ),
		fades = sampled_curve( fade_time, sampled_frames, step, s2 );
	return granulate_sampled( *this, event_frames( length, grains_per_second, time_scatter, get_sample_rate() ), sampled_frames, selection, lengths, fades, mod, false );
	}

Audio Audio::psola( Second length, const Function<Second, Second> & time_selection, const AudioMod & mod ) const
	{
	if( is_null() ) return Audio::create_null();
	const FrameRate sr = get_sample_rate();
	const auto freq = get_frequency_envelope();                                    // :617
	const float whole = std::ceil( time_to_frame( length ) );                      // :620
	if( !( length > 0 ) || !( whole < 2147483648.0f ) ) return Audio::create_null();
	const Frame selection_frames = Frame( whole );
	std::vector<float> s0;
	const SampledCurve selection = sampled_curve( time_selection, selection_frames, frame_to_time( 1 ), s0 );
	// :629-636: granulate's Functions read the sampled selection at time_to_frame( t ); granulate samples them at f * frame_to_time( 1 ) and
	// integrate_event_rate at f * ( 1.0f / sample rate ), the same float
	Frame sampled_frames = 0;
	if( !frame_of( length, sr, sampled_frames ) || sampled_frames < 1 ) return Audio::create_null();
	const float step = frame_to_time( 1 );
	std::vector<float> rate( static_cast<size_t>( sampled_frames ) ), picked( rate.size() ), lengths( rate.size() );
	for( Frame f = 0; f < sampled_frames; ++f )
		{
		Frame at = 0;
		if( !frame_of( Second( f * step ), sr, at ) || at >= selection_frames ) at = selection_frames - 1;      // (at <= f < selection_frames)
		picked[size_t( f )] = selection.at( at );
		rate[size_t( f )] = freq( picked[size_t( f )] );
		lengths[size_t( f )] = 2.0f / rate[size_t( f )];                           // :634: infinite where no pitch is found
		}
	std::vector<int64_t> frames( rate.size() );
	int64_t count = 0;
	if( flanhip_grains_events( sampled_frames, sr, rate.data(), 0.0f, nullptr, 0.0f, 0, frames.data(), sampled_frames, &count ) != FLANHIP_OK ) return Audio::create_null();
	frames.resize( static_cast<size_t>( count ) );
	return granulate_sampled( *this, frames, sampled_frames, SampledCurve{ &picked, 0.0f }, SampledCurve{ &lengths, 0.0f }, SampledCurve{ nullptr, 0.05f }, mod, true );
	}

// ---- silence removal and slicing (Audio/AudioTemporal.cpp:10-188, 301-546) ----------------------------------------------------
namespace {

// The detection on the device: the summary { count, first, last, 0 } and, if wanted, the chunk table
struct LoudScan
	{
	bool ok = false;
	int64_t summary[4] = { 0, -1, -1, 0 };
	std::vector<int32_t> chunks;                                               // [count][2]
	};

LoudScan loud_scan( const Audio & me, Amplitude level, Frame gap, bool want_table, const char * who )
	{
	LoudScan r;
	const int64_t ch = me.get_num_channels(), n = me.get_num_frames();
	const size_t ws_bytes = flanhip_loud_workspace_bytes( ch, n );
	if( ws_bytes == 0 )
		{
		std::cerr << "flan: " << who << " refused the shape: " << ch << " x " << n << std::endl;
		return r;
		}
	const float * d_x = me.device_data();
	if( !d_x ) return r;
	DeviceCall call( who );
	int64_t * d_summary = static_cast<int64_t*>( call.scratch( sizeof( r.summary ) ) );
	void * ws = call.workspace( ws_bytes );
	if( !call.ok() || !call.launch( flanhip_loud_summary_dev( d_x, ch, n, level, gap, d_summary, ws, nullptr ) ) || !call.sync() ) return r;
	if( !detail::download_to_host( r.summary, d_summary, sizeof( r.summary ) ) )      // the one read-back: the count sizes the table
		{
		std::cerr << "flan: " << who << ": download failed: " << flanhip_last_error() << std::endl;
		return r;
		}
	const int64_t count = r.summary[0];
	if( want_table && count > 0 )
		{
		r.chunks.resize( size_t( count ) * 2 );
		DeviceCall table( who );                                               // declared after `call`: its blocks go first, the workspace outlives the launch
		int32_t * d_chunks = static_cast<int32_t*>( table.scratch( sizeof( int32_t ) * r.chunks.size() ) );
		if( !table.ok() || !table.launch( flanhip_loud_chunks_dev( ch, n, gap, count, d_chunks, count, ws, nullptr ) ) || !table.sync() ) return r;
		if( !detail::download_to_host( r.chunks.data(), d_chunks, sizeof( int32_t ) * r.chunks.size() ) )
			{
			std::cerr << "flan: " << who << ": download failed: " << flanhip_last_error() << std::endl;
			return r;
			}
		}
	r.ok = true;
	return r;
	}

// get_loud_chunks_base (:10-86) up to its cuts: the chunks of `me` as events over `me` itself (join: placed as remove_silence joins them) and the
// offsets -2 * fade_ins[i].  false: nothing to return -- a null *this, nothing noisy, or a failure that has been reported
bool loud_events( const Audio & me, Amplitude level, Second minimum_gap, Second fade_in_time, bool join, EventTable & table, std::vector<Second> & offsets,
	const char * who )
	{
	if( me.is_null() ) return false;
	Frame gap = 0;
	if( !frame_of( minimum_gap, me.get_sample_rate(), gap ) )                  // :17
		{
		std::cerr << "flan: " << who << ": a minimum gap no frame holds" << std::endl;
		return false;
		}
	const LoudScan scan = loud_scan( me, level, gap, true, who );
	if( !scan.ok || scan.summary[0] == 0 ) return false;                       // :50
	const int64_t count = scan.summary[0];
	table.events.assign( size_t( count ), plain_event() );
	offsets.assign( size_t( count ) + 1, 0.0f );
	if( flanhip_loud_chunks_fades( me.get_num_frames(), me.get_sample_rate(), scan.chunks.data(), count, fade_in_time, join ? 1 : 0, table.events.data(),
			offsets.data() ) != FLANHIP_OK )
		{
		std::cerr << "flan: " << who << ": " << flanhip_last_error() << std::endl;
		return false;
		}
	for( flanhip_grain_event & e : table.events ) if( !point_at( me, e ) ) return false;
	return true;
	}

// every event of a table mixed alone from frame 0: cut_frames with its fades, the way granulate_sampled's general path makes a grain.  An empty
// event is a null Audio
std::vector<Audio> materialised( const char * who, const EventTable & table, Channel channels, FrameRate sample_rate )
	{
	std::vector<Audio> out;
	out.reserve( table.events.size() );
	for( flanhip_grain_event e : table.events )
		{
		e.o = 0;
		EventTable one;
		one.events.push_back( e );
		out.emplace_back( e.n > 0 ? mix_events( who, one, channels, sample_rate ) : Audio() );
		}
	return out;
	}

// Audio::join's places (AudioCombination.cpp:212-218, then mix's time_to_frame, :127-129) for events that are whole inputs of n frames
bool place_joined( EventTable & table, const std::vector<Second> & offsets, FrameRate sample_rate )
	{
	Second start_time = 0;
	for( size_t i = 0; i < table.events.size(); ++i )
		{
		Frame o = 0;
		if( !frame_of( start_time, sample_rate, o ) ) return false;
		table.events[i].o = o;
		start_time = start_time + table.events[i].n / sample_rate + offsets[i + 1];
		}
	return true;
	}

// split_at_times' frames (:416-429) through the C ABI; empty on a refusal, which is reported
std::vector<int32_t> split_frames_of( const Audio & me, const std::vector<Second> & times, const char * who )
	{
	std::vector<int32_t> frames( times.size() + 2 );
	int64_t count = 0;
	if( flanhip_split_frames( me.get_num_frames(), me.get_sample_rate(), times.data(), int64_t( times.size() ), frames.data(), int64_t( frames.size() ), &count ) != FLANHIP_OK )
		{
		std::cerr << "flan: " << who << ": " << flanhip_last_error() << std::endl;
		return {};
		}
	frames.resize( size_t( count ) );
	return frames;
	}

// split_with_lengths' times (:445-449) and split_with_equal_lengths' lengths (:458-459); false for a count no vector should hold
void lengths_to_times( std::vector<Second> & lengths )
	{
	for( Second & t : lengths ) if( t < 0 ) t = 0;
	for( size_t i = 1; i < lengths.size(); ++i ) lengths[i] = lengths[i - 1] + lengths[i];      // std::partial_sum in fp32
	}
bool equal_lengths( const Audio & me, Second slice_length, std::vector<Second> & lengths, const char * who )
	{
	const float count = std::ceil( me.get_length() / slice_length );
	if( !( count < float( 1 << 28 ) ) )
		{
		std::cerr << "flan: " << who << ": " << count << " slices" << std::endl;
		return false;
		}
	lengths.assign( size_t( std::max( count, 0.0f ) ), slice_length );
	return true;
	}

} // namespace

uint64_t Audio::random_seed() { return std::random_device()(); }

Audio Audio::modify_boundaries_frames( Frame start, Frame end ) const
	{
	if( is_null() ) return Audio::create_null();                                   // :101
	const int64_t out_frames = -int64_t( start ) + get_num_frames() + int64_t( end );      // :103
	if( out_frames <= 0 ) return Audio::create_null();
	if( out_frames > INT_MAX )
		{
		std::cerr << "flan: modify_boundaries: an output of " << out_frames << " frames" << std::endl;
		return Audio::create_null();
		}
	EventTable table;
	table.events.push_back( plain_event() );
	Frame o = 0;
	if( !frame_of( -frame_to_time( fFrame( start ) ), get_sample_rate(), o ) || !whole_event( *this, table.events[0] ) ) return Audio::create_null();      // :111
	table.events[0].o = o;
	return mix_events( "modify_boundaries", table, get_num_channels(), get_sample_rate(), out_frames );
	}

Audio Audio::modify_boundaries( Second start, Second end ) const
	{
	if( is_null() ) return Audio::create_null();
	Frame s = 0, e = 0;
	if( !frame_of( start, get_sample_rate(), s ) || !frame_of( end, get_sample_rate(), e ) ) return Audio::create_null();      // :121
	return modify_boundaries_frames( s, e );
	}

Audio Audio::remove_edge_silence( Amplitude non_silent_level, Second fade_time ) const
	{
	if( is_null() ) return Audio::create_null();
	const LoudScan scan = loud_scan( *this, non_silent_level, 0, false, "remove_edge_silence" );      // :129-147: the summary's first and last
	if( !scan.ok ) return Audio::create_null();
	int32_t cut[4];
	if( flanhip_edge_silence_cut( get_num_frames(), get_sample_rate(), scan.summary[1], scan.summary[2], fade_time, cut ) != FLANHIP_OK )
		{
		std::cerr << "flan: remove_edge_silence: " << flanhip_last_error() << std::endl;
		return Audio::create_null();
		}
	return cut_frames( cut[0], cut[1], cut[2], cut[3] );                          // :152
	}

std::vector<Audio> Audio::get_loud_chunks( Amplitude non_silent_level, Second minimum_gap, Second fade_in_time ) const
	{
	EventTable table;
	std::vector<Second> offsets;
	if( !loud_events( *this, non_silent_level, minimum_gap, fade_in_time, false, table, offsets, "get_loud_chunks" ) ) return {};
	return materialised( "get_loud_chunks", table, get_num_channels(), get_sample_rate() );
	}

Audio Audio::remove_silence( Amplitude non_silent_level, Second minimum_gap, Second fade_in_time ) const
	{
	EventTable table;
	std::vector<Second> offsets;
	if( !loud_events( *this, non_silent_level, minimum_gap, fade_in_time, true, table, offsets, "remove_silence" ) ) return Audio::create_null();
	return mix_events( "remove_silence", table, get_num_channels(), get_sample_rate() );
	}

Audio Audio::remove_silence_unfused( Amplitude non_silent_level, Second minimum_gap, Second fade_in_time ) const
	{
	EventTable table;
	std::vector<Second> offsets;
	if( !loud_events( *this, non_silent_level, minimum_gap, fade_in_time, false, table, offsets, "remove_silence" ) ) return Audio::create_null();
	const std::vector<Audio> chunks = materialised( "remove_silence", table, get_num_channels(), get_sample_rate() );
	return Audio::join( pointers_to( chunks ), offsets );                          // :170-171
	}

Audio Audio::reverse() const
	{
	if( is_null() ) return Audio::create_null();                                   // :177
	const float * d_x = device_data();
	if( !d_x ) return Audio::create_null();
	return audio_call( "reverse", get_format(), true, detail::kNoWorkspace, [&]( float * out, void * )
		{ return flanhip_audio_reverse_dev( d_x, get_num_channels(), get_num_frames(), out, nullptr ); } );
	}

Audio Audio::iterate( int32_t num_iterations, Second crossfade_time, const AudioMod & mod, bool feedback ) const
	{
	if( is_null() ) return Audio::create_null();                                   // :308-309
	if( num_iterations < 1 ) return Audio::create_null();
	if( mod.is_null() ) return Audio::join( std::vector<const Audio *>( size_t( num_iterations ), this ), -crossfade_time );      // :312-313
	std::vector<Audio> modified;                                                   // :316-321, on the calling thread in order
	modified.reserve( size_t( num_iterations ) );
	for( int32_t i = 0; i < num_iterations; ++i )
		{
		Audio input = i > 0 && feedback ? modified.back().copy() : copy();
		mod( input, i * get_length() );
		modified.emplace_back( std::move( input ) );
		}
	return Audio::join( modified, -crossfade_time );                               // :323
	}

Audio Audio::delay( Second added_length, const Function<Second, Second> & delay_time, const Function<Second, float> & decay, const AudioMod & mod ) const
	{
	if( is_null() ) return Audio::create_null();                                   // :333
	added_length = std::max( 0.0f, added_length );                                 // :335-336
	const Second length = get_length() + added_length;
	Frame frames = 0;
	if( !frame_of( length, get_sample_rate(), frames ) || frames < 1 ) return Audio::create_null();
	const auto delay_time_sampled = delay_time.sample( 0, frames, frame_to_time( 1 ) );      // :338-339
	const auto decay_sampled = decay.sample( 0, frames, frame_to_time( 1 ) );
	const FrameRate sr = get_sample_rate();
	const auto at = [frames, sr]( const auto & sampled, Second t )                // sampled[ time_to_frame( t ) ], held inside the samples
		{
		if( sampled.is_constant() ) return sampled.get_constant();
		Frame f = 0;
		if( !frame_of( t, sr, f ) ) f = 0;
		return sampled.get_vector()[size_t( std::clamp( f, 0, frames - 1 ) )];
		};
	const Function<Second, float> events_per_second( [&]( Second t )                // :341-346
		{
		const Second delay_time_c = at( delay_time_sampled, t );
		if( delay_time_c <= 0 ) return 1.0f / float( sr );
		return 1.0f / delay_time_c;
		} );
	const AudioMod delay_mod( [&]( Audio & in, Second t )                          // :348-358
		{
		if( t == 0 ) return;
		if( !mod.is_null() ) mod( in, t );
		in.modify_volume_in_place( at( decay_sampled, t ) );                       // one fp32 product per sample by a constant
		} );
	return texture( length, events_per_second, 0, delay_mod, true );                 // :360
	}

std::vector<Audio> Audio::split_at_times( std::vector<Second> split_times, Second fade ) const
	{
	if( is_null() ) return {};                                                     // :414
	Frame fade_frames = 0;
	if( !frame_of( fade, get_sample_rate(), fade_frames ) ) return {};             // :416
	const std::vector<int32_t> frames = split_frames_of( *this, split_times, "split_at_times" );
	std::vector<Audio> outs;
	for( size_t i = 0; i + 1 < frames.size(); ++i ) outs.emplace_back( cut_frames( frames[i], frames[i + 1], fade_frames, fade_frames ) );      // :434
	return outs;
	}

std::vector<Audio> Audio::split_with_lengths( std::vector<Second> split_lengths, Second fade ) const
	{
	lengths_to_times( split_lengths );                                             // :445-449
	return split_at_times( std::move( split_lengths ), fade );
	}

std::vector<Audio> Audio::split_with_equal_lengths( Second slice_length, Second fade ) const
	{
	if( is_null() || !( slice_length > 0 ) ) return {};                            // :458
	std::vector<Second> lengths;
	if( !equal_lengths( *this, slice_length, lengths, "split_with_equal_lengths" ) ) return {};
	return split_with_lengths( std::move( lengths ), fade );
	}

Audio Audio::rearrange( Second slice_length, Second fade, uint64_t seed ) const
	{
	if( is_null() ) return Audio::create_null();                                   // :468
	Frame fade_frames = 0;
	std::vector<Second> times;
	if( !( slice_length + fade > 0 ) || !frame_of( fade, get_sample_rate(), fade_frames ) || !equal_lengths( *this, slice_length + fade, times, "rearrange" ) )
		return Audio::create_null();                                               // :471: split_with_equal_lengths( slice_length + fade, fade )
	lengths_to_times( times );
	const std::vector<int32_t> frames = split_frames_of( *this, times, "rearrange" );
	if( frames.size() < 3 ) return Audio::create_null();                           // :472-473: fewer than 2 pieces
	const size_t count = frames.size() - 2;                                        // :475: without the last piece
	std::vector<int32_t> order( count ), start( count ), end( count ), fades( count, fade_frames );
	if( flanhip_rearrange_order( int64_t( count ), seed, order.data() ) != FLANHIP_OK ) return Audio::create_null();
	for( size_t i = 0; i < count; ++i ) { start[i] = frames[size_t( order[i] )]; end[i] = frames[size_t( order[i] ) + 1]; }
	EventTable table;
	table.events.assign( count, plain_event() );
	if( flanhip_grains_cut_frames( get_num_frames(), int64_t( count ), start.data(), end.data(), fades.data(), fades.data(), table.events.data() ) != FLANHIP_OK
		|| !place_joined( table, std::vector<Second>( count + 1, -fade ), get_sample_rate() ) ) return Audio::create_null();      // :481
	for( flanhip_grain_event & e : table.events ) if( !point_at( *this, e ) ) return Audio::create_null();
	return mix_events( "rearrange", table, get_num_channels(), get_sample_rate() );
	}

Audio Audio::random_chunks( Second length, const Function<Second, Second> & chunk_length, const Function<Second, Second> & fade, const AudioMod & mod,
	uint64_t seed ) const
	{
	if( is_null() || !( length > 0 ) ) return Audio::create_null();                // :491
	const FrameRate sr = get_sample_rate();
	const int64_t loop_frames = flanhip_random_chunks_frames( sr, length );
	if( loop_frames < 1 || loop_frames >= INT_MAX ) return Audio::create_null();
	std::vector<float> lengths, fades;                                             // the Functions at frame_to_time( f ) (:505, :519)
	if( !chunk_length.is_constant() )
		{
		lengths.resize( size_t( loop_frames ) );
		detail::for_each_index( 0, int( loop_frames ), chunk_length.get_execution_policy(), [&]( int f ){ lengths[size_t( f )] = chunk_length( frame_to_time( fFrame( f ) ) ); } );
		}
	if( !fade.is_constant() )
		{
		fades.resize( size_t( loop_frames ) + 1 );
		detail::for_each_index( 0, int( loop_frames ) + 1, fade.get_execution_policy(), [&]( int f ){ fades[size_t( f )] = fade( frame_to_time( fFrame( f ) ) ); } );
		}
	const float * lp = lengths.empty() ? nullptr : lengths.data(), * fp = fades.empty() ? nullptr : fades.data();
	const float ls = chunk_length.is_constant() ? chunk_length.get_constant() : 0.0f, fs = fade.is_constant() ? fade.get_constant() : 0.0f;
	int64_t count = 0;
	EventTable table;
	std::vector<int32_t> starts;
	std::vector<Second> offsets;
	bool planned = flanhip_random_chunks_plan( get_num_frames(), sr, length, lp, ls, fp, fs, seed, nullptr, nullptr, nullptr, 0, &count ) == FLANHIP_OK;
	if( planned )
		{
		table.events.assign( size_t( count ), plain_event() );
		starts.resize( size_t( count ) );
		offsets.resize( size_t( count ) + 1 );
		planned = flanhip_random_chunks_plan( get_num_frames(), sr, length, lp, ls, fp, fs, seed, table.events.data(), starts.data(), offsets.data(), count, &count ) == FLANHIP_OK;
		}
	if( !planned )
		{
		std::cerr << "flan: random_chunks: " << flanhip_last_error() << std::endl;
		return Audio::create_null();
		}
	for( flanhip_grain_event & e : table.events ) if( !point_at( *this, e ) ) return Audio::create_null();
	if( mod.is_null() ) return mix_events( "random_chunks", table, get_num_channels(), sr );       // fused: every chunk read from *this in the mix
	std::vector<Audio> chunks = materialised( "random_chunks", table, get_num_channels(), sr );   // :529-539
	for( size_t i = 0; i < chunks.size(); ++i ) mod( chunks[i], frame_to_time( fFrame( starts[i] ) ) );
	return Audio::join( pointers_to( chunks ), offsets );                          // :545
	}

// Audio/AudioSynthesis.cpp:151-268.  The spectrum's magnitudes and phases and the frequency curve are made here; the table (one inverse real FFT
// of 2^spectrum_size_power points), the resampler loop over it and set_volume( 1 ) run on the device without coming back in between
Audio Audio::synthesize_spectrum( Second length, const Function<Second, Frequency> & freq, const Function<Harmonic, Frequency> & spread,
	const Function<Harmonic, Amplitude> & harmonic_scale, const Function<Frequency, Amplitude> & peak_distribution, int fundamental_power,
	int spectrum_size_power, Channel num_channels, Second granularity_time, const std::vector<Radian> * phases )
	{
	if( length <= 0 || fundamental_power <= 0 || spectrum_size_power <= 0 || fundamental_power > spectrum_size_power || granularity_time <= 0 )
		return Audio::create_null();                                               // :163-168
	const FrameRate sr = 48000.0f;                                                 // the table's, create_empty_with_frames' default (:179)
	AudioBuffer::Format format;                                                    // :224-228
	format.num_channels = num_channels; format.sample_rate = sr;
	Frame granularity = 0;
	const int64_t bins = flanhip_spectrum_bins( spectrum_size_power, fundamental_power, nullptr, nullptr, 0 );
	if( !frame_of( length, sr, format.num_frames ) || !frame_of( granularity_time, sr, granularity ) || format.num_frames < 1 || granularity < 1
		|| num_channels < 1 || bins < 1 || flanhip_spectrum_table_workspace_bytes( spectrum_size_power ) == 0 || ( phases && int64_t( phases->size() ) != bins ) )
		{
		std::cerr << "flan: synthesize_spectrum refused: 2^" << spectrum_size_power << " table frames (6 ... 22 are served), " << format.num_frames
		          << " output frames, a granularity of " << granularity << " frames, " << num_channels << " channels"
		          << ( phases && int64_t( phases->size() ) != bins ? ", phases that are not one per bin" : "" ) << std::endl;
		return Audio::create_null();
		}
	const Frame n = format.num_frames;

	// :185-210: per-harmonic spread and scale, then one magnitude per bin with a harmonic
	std::vector<int32_t> harmonic( static_cast<size_t>( bins ) );
	std::vector<float> bin_frequency( harmonic.size() );
	flanhip_spectrum_bins( spectrum_size_power, fundamental_power, harmonic.data(), bin_frequency.data(), bins );
	const Harmonic num_harmonics = flanhip_spectrum_num_harmonics( fundamental_power );
	const Frequency fundamental = Frequency( std::pow( 2, fundamental_power ) );
	std::vector<Amplitude> harmonic_scale_sampled( static_cast<size_t>( num_harmonics ) ), spread_sampled( harmonic_scale_sampled.size() );
	detail::for_each_index( 0, num_harmonics, harmonic_scale.get_execution_policy(), [&]( int h ){ harmonic_scale_sampled[size_t( h )] = harmonic_scale( h + 1 ); } );
	detail::for_each_index( 0, num_harmonics, spread.get_execution_policy(), [&]( int h ){ spread_sampled[size_t( h )] = spread( h + 1 ); } );
	detail::StagingVector<float> mag( harmonic.size() ), theta( harmonic.size() );
	detail::for_each_index( 0, int( bins ), peak_distribution.get_execution_policy(), [&]( int bin )
		{
		const int h = harmonic[size_t( bin )];
		mag[size_t( bin )] = 0.0f;                                                 // (the reference leaves a skipped bin uninitialised)
		if( h <= 0 || h > num_harmonics ) return;
		const Frequency epsilon = 0.001f;
		const Frequency mean = fundamental * h;
		const Frequency sd = spread_sampled[size_t( h - 1 )];
		const Frequency x = bin_frequency[size_t( bin )];
		mag[size_t( bin )] = ( sd <= epsilon ? x : peak_distribution( ( x - mean ) / sd ) / sd ) * harmonic_scale_sampled[size_t( h - 1 )];
		} );
	if( phases ) std::copy( phases->begin(), phases->end(), &theta[0] );
	else
		{
		std::random_device rd;                                                     // :182-183
		flanhip_spectrum_phases( rd(), harmonic.data(), bins, &theta[0] );
		}

	// freq at every output frame (a block reads the entry of the frame it starts on, :243); a constant is one entry
	std::vector<float> freq_v( freq.is_constant() ? size_t( 1 ) : size_t( n ) );
	if( freq.is_constant() ) freq_v[0] = freq.get_constant();
	else detail::for_each_index( 0, n, freq.get_execution_policy(), [&]( int x ){ freq_v[size_t( x )] = freq( fFrame( x ) / sr ); } );

	const size_t ws_bytes = flanhip_audio_synthesize_spectrum_workspace_bytes( spectrum_size_power, fundamental_power, num_channels, n, granularity, freq_v.data(),
		int64_t( freq_v.size() ) );
	if( ws_bytes == 0 )
		{
		std::cerr << "flan: synthesize_spectrum refused: " << flanhip_last_error() << std::endl;
		return Audio::create_null();
		}
	const DeviceArg d_mag = upload_values( mag ), d_theta = upload_values( theta );
	return audio_call( "synthesize_spectrum", format, d_mag.ok && d_theta.ok, ws_bytes, [&]( float * d_out, void * ws )
		{
		return flanhip_audio_synthesize_spectrum_dev( d_mag.ptr(), d_theta.ptr(), spectrum_size_power, fundamental_power, num_channels, n, granularity,
			freq_v.data(), int64_t( freq_v.size() ), d_out, ws, nullptr );
		} );
	}

// ---- the rest of Audio/AudioVolume.cpp (:15-30, 69-188, 280-321), the energies and the amplitude envelope of Audio/AudioInformation.cpp
// (:121-136, 320-363) and the oscillator and white noise of Audio/AudioSynthesis.cpp (:25-89); DESIGN.md 4.26 ------------------------------

Audio Audio::ring_modulate( const Audio & other ) const
	{
	if( is_null() || other.is_null() ) return Audio::create_null();                // :19
	const float * d_x = device_data();
	const float * d_o = other.device_data();
	if( !d_x || !d_o ) return Audio::create_null();
	return audio_call( "ring_modulate", get_format(), true, detail::kNoWorkspace, [&]( float * out, void * )
		{ return flanhip_audio_ring_modulate_dev( d_x, get_num_channels(), get_num_frames(), d_o, other.get_num_channels(), other.get_num_frames(), out, nullptr ); } );
	}

Audio Audio::fade( Second start, Second end, const Interpolator & interp ) const
	{
	if( is_null() ) return Audio::create_null();                                   // :75
	return fade_frames( Frame( time_to_frame( start ) ), Frame( time_to_frame( end ) ), interp );
	}

Audio & Audio::fade_in_place( Second start, Second end, const Interpolator & interp )
	{
	if( is_null() ) { std::cout << "Null input" << std::endl; return *this; }     // :85
	return fade_frames_in_place( Frame( time_to_frame( start ) ), Frame( time_to_frame( end ) ), interp );
	}

Audio Audio::fade_frames( Frame start, Frame end, const Interpolator & interp ) const
	{
	if( is_null() ) return Audio::create_null();                                   // :96
	int32_t plan[2];
	if( flanhip_fade_frames_plan( get_num_frames(), start, end, plan ) != FLANHIP_OK ) return Audio::create_null();      // :111-118
	start = plan[0]; end = plan[1];
	if( start == 0 && end == 0 ) return copy();                                    // :119
	const float * d_x = device_data();
	if( !d_x ) return Audio::create_null();
	// the interpolator where the two loops evaluate it (:125, :130): exact for every one, named or callable
	detail::StagingVector<float> start_gain( static_cast<size_t>( start ) ), end_gain( static_cast<size_t>( end ) );
	for( Frame frame = 0; frame < start; ++frame ) start_gain[size_t( frame )] = interp( float( frame ) / start );
	for( Frame frame = 0; frame < end; ++frame ) end_gain[size_t( frame )] = interp( float( frame ) / end );
	const DeviceArg s = start ? upload_values( start_gain ) : DeviceArg(), e = end ? upload_values( end_gain ) : DeviceArg();
	return audio_call( "fade_frames", get_format(), s.ok && e.ok, detail::kNoWorkspace, [&]( float * out, void * )
		{ return flanhip_audio_fade_dev( d_x, get_num_channels(), get_num_frames(), s.ptr(), start, e.ptr(), end, out, nullptr ); } );
	}

Audio & Audio::fade_frames_in_place( Frame start, Frame end, const Interpolator & interp )
	{
	if( is_null() ) { std::cout << "Null input" << std::endl; return *this; }     // :108
	Audio out = fade_frames( start, end, interp );
	if( !out.is_null() ) *this = std::move( out );
	return *this;
	}

Audio Audio::invert_phase() const
	{
	if( is_null() ) return Audio::create_null();                                   // :140
	const float * d_x = device_data();
	if( !d_x ) return Audio::create_null();
	return audio_call( "invert_phase", get_format(), true, detail::kNoWorkspace, [&]( float * out, void * )
		{ return flanhip_audio_gain_dev( d_x, get_num_channels(), get_num_frames(), nullptr, -1.0f, out, nullptr ); } );
	}

Audio Audio::waveshape( const Function<std::pair<Second, Sample>, Sample> & shaper, uint16_t oversample_factor ) const
	{
	if( is_null() ) return Audio::create_null();                                   // :151
	Audio oversampled = resample( get_sample_rate() * oversample_factor );         // :153
	if( oversampled.is_null() ) return Audio::create_null();
	std::vector<float> & samples = oversampled.get_buffer();                       // the one download; the host copy is the truth from here
	for( Channel channel = 0; channel < oversampled.get_num_channels(); ++channel )           // :154-164
		detail::for_each_index( 0, oversampled.get_num_frames(), shaper.get_execution_policy(), [&]( int frame )
			{
			Sample & s = samples[oversampled.get_buffer_pos( channel, frame )];
			s = shaper( std::pair<Second, Sample>( oversampled.frame_to_time( frame ), s ) );
			} );
	return oversampled.resample( get_sample_rate() );                              // :165
	}

Audio Audio::add_moisture( const Function<Second, Amplitude> & amount, const Function<Second, Frequency> & frequency, const Function<Second, float> & skew,
	const Waveform & waveform ) const
	{
	if( is_null() ) return Audio::create_null();
	const Frame n = get_num_frames();
	const float sr = get_sample_rate();
	if( waveform.kind() < 0 )                                                      // :175-187 as written, on the host
		{
		const auto amount_sampled = amount.sample( 0, n, 1.0f / sr ), frequency_sampled = frequency.sample( 0, n, 1.0f / sr ), skew_sampled = skew.sample( 0, n, 1.0f / sr );
		const auto at = [n]( const auto & sampled, Frame i ) { return sampled.is_constant() ? sampled.get_constant() : sampled.get_vector()[size_t( std::clamp( i, 0, n - 1 ) )]; };
		return waveshape( Function<std::pair<Second, Sample>, Sample>( [&]( std::pair<Second, Sample> ts ) -> Sample
			{
			const Frame i = Frame( time_to_frame( ts.first ) );
			const float amount_c = at( amount_sampled, i ), frequency_c = at( frequency_sampled, i ), skew_c = at( skew_sampled, i );
			const float power = ts.second >= 0 ? std::pow( ts.second, skew_c ) : -std::pow( -ts.second, skew_c );
			return ts.second + amount_c * ts.second * waveform( pi2 * frequency_c * power );
			}, waveform.get_execution_policy() ) );
		}
	const Audio oversampled = resample( sr * uint16_t( 4 ) );                       // :153 with the default factor
	if( oversampled.is_null() ) return Audio::create_null();
	const float * d_over = oversampled.device_data();
	if( !d_over ) return Audio::create_null();
	const DeviceArg a = upload_curve( amount, n, 1.0f / sr ), f = upload_curve( frequency, n, 1.0f / sr ), k = upload_curve( skew, n, 1.0f / sr );
	const Audio shaped = audio_call( "add_moisture", oversampled.get_format(), a.ok && f.ok && k.ok, detail::kNoWorkspace, [&]( float * out, void * )
		{
		return flanhip_audio_moisture_dev( d_over, oversampled.get_num_channels(), oversampled.get_num_frames(), oversampled.get_sample_rate(), n, sr,
			a.ptr(), a.scalar, f.ptr(), f.scalar, k.ptr(), k.scalar, waveform.kind(), out, nullptr );
		} );
	if( shaped.is_null() ) return Audio::create_null();
	return shaped.resample( sr );                                                  // :165
	}

Audio Audio::apply_adsr_envelope( Second attack_time, Second decay_time, Second sustain_time, Second release_time, Amplitude sustain_level,
	float attack_exponent, float decay_exponent, float release_exponent ) const
	{
	return modify_volume( ADSR( attack_time, decay_time, sustain_time, release_time, sustain_level, attack_exponent, decay_exponent, release_exponent ) );
	}

Audio Audio::apply_ar_envelope( Second attack_time, Second release_time, float attack_exponent, float release_exponent ) const
	{
	return modify_volume( ADSR( attack_time, 0, 0, release_time, 1, attack_exponent, 1, release_exponent ) );
	}

std::vector<float> Audio::get_total_energy() const
	{
	if( is_null() ) return std::vector<float>();
	const float * d_x = device_data();
	const size_t ws_bytes = flanhip_audio_energy_workspace_bytes( get_num_channels(), get_num_frames() );
	if( !d_x || ws_bytes == 0 ) return std::vector<float>();
	std::vector<float> energies( static_cast<size_t>( get_num_channels() ) );
	if( !wavelengths_call( "get_total_energy", energies, ws_bytes, [&]( float * d_out, void * ws )
		{ return flanhip_audio_energy_dev( d_x, get_num_channels(), get_num_frames(), d_out, ws, nullptr ); } ) ) return std::vector<float>();
	return energies;
	}

std::vector<float> Audio::get_energy_difference( const Audio & other ) const
	{
	if( is_null() || other.is_null() ) return std::vector<float>();
	const Audio resampled = get_sample_rate() == other.get_sample_rate() ? Audio() : other.resample( get_sample_rate() );      // :133
	const Audio * sr_correct_source = get_sample_rate() == other.get_sample_rate() ? &other : &resampled;
	return Audio::mix( std::vector<const Audio *>{ this, sr_correct_source }, { 0, 0 }, { 1, -1 } ).get_total_energy();        // :135
	}

Function<Second, Amplitude> Audio::get_amplitude_envelope( Second window_width ) const
	{
	if( is_null() ) return 0;                                                      // :324
	if( window_width <= 0 ) return 0;                                              // :326
	const Audio mono = convert_to_mono();                                          // :328
	const float * d_mono = mono.is_null() ? nullptr : mono.device_data();
	if( !d_mono ) return 0;
	const Audio rectified = audio_call( "get_amplitude_envelope", mono.get_format(), true, detail::kNoWorkspace, [&]( float * out, void * )
		{ return flanhip_audio_rectify_dev( d_mono, 1, mono.get_num_frames(), out, nullptr ); } );        // :331-333
	if( rectified.is_null() ) return 0;
	const fFrame window_width_frames = time_to_frame( window_width );              // :335
	const Frame window_frames = Frame( window_width_frames );                      // :337: create_empty_with_frames takes a Frame
	if( window_frames <= 0 ) return 0;
	std::vector<float> window( static_cast<size_t>( window_frames ) );
	float hann_integral = 0;
	for( Frame i = 0; i < window_frames; ++i )                                      // :339-343
		{
		const float x = float( i ) / ( window_width_frames - 1 );
		// Windows::hann (WindowFunctions.cpp:10-13): the fp32 argument, then the DOUBLE cos its unqualified call picks, narrowed on return
		window[size_t( i )] = float( 0.5 * ( 1.0 - std::cos( double( 2.0f * pi * x ) ) ) );
		hann_integral += window[size_t( i )];
		}
	const Audio hann_window = Audio::create_from_buffer( std::move( window ), 1, get_sample_rate() );
	Audio convolved = rectified.convolve( hann_window, false );                    // :345
	if( convolved.is_null() ) return 0;
	convolved.modify_volume_in_place( pi / 2.0f / hann_integral );                 // :346
	std::vector<float> ys = convolved.get_buffer();                                // :350
	return Function<Second, Amplitude>( [ys = std::move( ys ), sr = get_sample_rate()]( float t )      // :351-363
		{
		const float x = t * sr;
		if( 0 <= x && x < ys.size() - 1 )
			{
			const Frame x1 = Frame( std::floor( x ) );
			const float y1 = ys[size_t( x1 )];
			const float y2 = ys[size_t( x1 ) + 1];
			return y1 + ( y2 - y1 ) * ( x - x1 );
			}
		else return 0.0f;
		} );
	}

Audio Audio::synthesize_waveform( const Waveform & wave, Second length, const Function<Second, Frequency> & freq, FrameRate sample_rate, int oversample )
	{
	int64_t n_in = 0;
	double in_sample_rate = 0;
	const int64_t num_frames = flanhip_synthesize_waveform_frames( length, sample_rate, oversample, &n_in, &in_sample_rate );      // :33-44
	if( num_frames <= 0 ) return Audio::create_null();
	AudioBuffer::Format format;
	format.num_channels = 1;
	format.num_frames = Frame( num_frames );
	format.sample_rate = sample_rate;
	const DeviceArg f = upload_curve( freq, Frame( n_in ), float( 1.0f / in_sample_rate ) );     // :46 (a float over a double, narrowed by sample's float scale)
	if( wave.kind() >= 0 )
		{
		const size_t ws_bytes = flanhip_audio_synthesize_waveform_workspace_bytes( length, sample_rate, oversample );
		if( ws_bytes == 0 ) return Audio::create_null();
		return audio_call( "synthesize_waveform", format, f.ok, ws_bytes, [&]( float * out, void * ws )
			{ return flanhip_audio_synthesize_waveform_dev( wave.kind(), f.ptr(), f.scalar, length, sample_rate, oversample, out, ws, nullptr ); } );
		}
	// any other wave: the phases come to the host, the wave is evaluated there under its policy (:61-62), the samples go back for the chain
	const size_t ws_bytes = flanhip_osc_workspace_bytes( n_in );
	if( ws_bytes == 0 || !f.ok ) return Audio::create_null();
	detail::StagingVector<float> wave_samples( static_cast<size_t>( n_in ) );
	{
	std::vector<float> phases( static_cast<size_t>( n_in ) );
	if( !wavelengths_call( "synthesize_waveform", phases, ws_bytes, [&]( float * d_phases, void * ws )
		{ return flanhip_osc_phase_dev( f.ptr(), f.scalar, n_in, in_sample_rate, d_phases, nullptr, -1, ws, nullptr ); } ) ) return Audio::create_null();
	detail::for_each_index( 0, int( n_in ), wave.get_execution_policy(), [&]( int i ){ wave_samples[size_t( i )] = wave( phases[size_t( i )] ); } );
	}
	const DeviceArg w = upload_values( wave_samples );
	return audio_call( "synthesize_waveform", format, w.ok, detail::kNoWorkspace, [&]( float * out, void * )
		{ return flanhip_oneshot_resample_dev( w.ptr(), n_in, in_sample_rate, double( sample_rate ), out, num_frames, nullptr ); } );      // :65-66
	}

Audio Audio::synthesize_white_noise( Second length, FrameRate sample_rate, int oversample, uint64_t seed )
	{
	if( oversample < 1 || length <= 0 || sample_rate <= 0 ) return Audio::create_null();      // :77-78
	Audio out = Audio::create_empty_with_length( length, 1, sample_rate * oversample );       // :84
	if( out.is_null() ) return Audio::create_null();
	if( flanhip_white_noise_draw( seed, out.get_num_frames(), out.get_buffer().data() ) != FLANHIP_OK ) return Audio::create_null();      // :80-86
	return out.resample( sample_rate );                                            // :88
	}

} // namespace flan
