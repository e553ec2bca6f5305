// Wavetable.cpp -- flan::Wavetable over the C ABI (include/flanhip.h, flanhip_wavetable_*): the waveform starts on the host, the table, its
// synthesis and its edits on the device.  The reference is src/flan/Wavetable.cpp; line numbers below are its.
#include "flan/Wavetable.h"

#include <algorithm>
#include <cmath>
#include <iostream>

#include "device_call.h"

namespace flan {

namespace {
using detail::DeviceCall;

int snap_code( Wavetable::SnapMode m ) { return m == Wavetable::SnapMode::Zero ? FLANHIP_WAVETABLE_SNAP_ZERO : m == Wavetable::SnapMode::Level ? FLANHIP_WAVETABLE_SNAP_LEVEL : FLANHIP_WAVETABLE_SNAP_NONE; }
int pitch_code( Wavetable::PitchMode m ) { return m == Wavetable::PitchMode::Local ? FLANHIP_WAVETABLE_PITCH_LOCAL : m == Wavetable::PitchMode::Global ? FLANHIP_WAVETABLE_PITCH_GLOBAL : FLANHIP_WAVETABLE_PITCH_NONE; }

// get_waveform_starts (:134-218); an empty result makes a null Wavetable
std::vector<std::vector<Frame>> get_waveform_starts( const Audio & source, Wavetable::SnapMode snap_mode, Wavetable::PitchMode pitch_mode, Frame wavelength,
	float snap_ratio, Frame fixed_frame, std::atomic<bool> & canceller )
	{
	const std::vector<std::vector<Frame>> none;
	if( source.is_null() ) return none;                                          // :144-146
	if( fixed_frame < 1 ) return none;
	if( snap_ratio <= 0 || snap_ratio >= .95 ) return none;

	const Audio lp_source = pitch_mode != Wavetable::PitchMode::None ? source.filter_1pole_lowpass( 4000, 2 ) : Audio();      // :148 (read in the pitch modes only)
	if( pitch_mode != Wavetable::PitchMode::None && lp_source.is_null() ) return none;

	std::vector<std::vector<Frame>> waveform_starts( size_t( source.get_num_channels() ) );
	const Frame ac_granularity = 128;                                            // :153
	for( Channel channel = 0; channel < source.get_num_channels(); ++channel )
		{
		std::vector<fFrame> local_wavelengths;
		Frame global_wavelength = 0;
		if( pitch_mode != Wavetable::PitchMode::None )
			{
			local_wavelengths = lp_source.get_local_wavelengths( channel, 0, -1, wavelength, ac_granularity, 1, 32, canceller );   // :161
			global_wavelength = Frame( lp_source.get_average_wavelength( local_wavelengths, .2f, 64 ) );                         // :162, truncated
			if( pitch_mode == Wavetable::PitchMode::Global && global_wavelength == -1 )
				pitch_mode = Wavetable::PitchMode::None;                             // :163-164: the parameter itself, so later channels keep it
			}
		if( canceller ) return none;
		const float * row = source.get_sample_pointer( channel, 0 );                // the unfiltered source (:174-176)
		auto walk = [&]( Frame * out, int64_t capacity, int64_t * count )
			{
			return flanhip_wavetable_starts( row, source.get_num_frames(), local_wavelengths.data(), int64_t( local_wavelengths.size() ), global_wavelength,
				snap_code( snap_mode ), pitch_code( pitch_mode ), snap_ratio, fixed_frame, nullptr, out, capacity, count );
			};
		int64_t count = 0;
		if( !detail::report( walk( nullptr, 0, &count ), "Wavetable (waveform starts)" ) ) return none;
		waveform_starts[size_t( channel )].resize( size_t( count ) );
		if( !detail::report( walk( waveform_starts[size_t( channel )].data(), count, &count ), "Wavetable (waveform starts)" ) ) return none;
		}
	return waveform_starts;
	}

// resample_waveforms (:67-132) on the device
Audio resample_waveforms( const Audio & source, const std::vector<std::vector<Frame>> & waveform_starts, Frame wavelength )
	{
	if( source.is_null() || waveform_starts.empty() ) return Audio();           // :70-73 (the constructor's null, without the reference's line on stdout)
	std::vector<Frame> flat;
	std::vector<int64_t> counts;
	for( const auto & w : waveform_starts )
		{
		if( w.empty() ) return Audio();
		flat.insert( flat.end(), w.begin(), w.end() );
		counts.push_back( int64_t( w.size() ) );
		}
	const Channel ch = source.get_num_channels();
	if( size_t( ch ) != waveform_starts.size() ) return Audio();
	const int64_t slots = flanhip_wavetable_slots( counts.data(), ch );
	const size_t ws_bytes = flanhip_wavetable_resample_workspace_bytes( ch, source.get_num_frames(), flat.data(), counts.data(), wavelength );
	if( ws_bytes == 0 || slots * int64_t( wavelength ) > INT32_MAX )
		{
		std::cerr << "flan: Wavetable refused: " << flanhip_last_error() << std::endl;
		return Audio();
		}
	const float * d_x = source.device_data();
	if( !d_x ) return Audio();
	AudioBuffer::Format f = source.get_format();                                  // :76-80
	f.num_frames = Frame( slots * wavelength );
	AudioBuffer out = detail::device_call<AudioBuffer, float>( "Wavetable", f, size_t( ch ) * size_t( f.num_frames ), true, ws_bytes, [&]( float * d_table, void * ws )
		{ return flanhip_wavetable_resample_dev( d_x, ch, source.get_num_frames(), flat.data(), counts.data(), wavelength, d_table, nullptr, ws, nullptr ); } );
	return out.is_null() ? Audio() : Audio( std::move( out ) );
	}

}

Wavetable::Wavetable( const Audio & source, SnapMode snap_mode, PitchMode pitch_mode, Frame _wavelength, float snap_ratio, Frame fixed, flan_CANCEL_ARG_CPP )
	: wavelength( _wavelength )
	, num_source_frames( source.get_num_frames() )
	, waveform_starts( get_waveform_starts( source, snap_mode, pitch_mode, _wavelength, snap_ratio, fixed, canceller ) )
	, table( resample_waveforms( source, waveform_starts, _wavelength ) )
	{
	}

Wavetable::Wavetable( const Function<Second, Amplitude> & f, int num_waves, Frame _wavelength, flan_CANCEL_ARG_CPP )
	: wavelength( _wavelength )
	, num_source_frames( num_waves )
	, waveform_starts( 1, std::vector<Frame>( size_t( std::max( num_waves, 0 ) ) ) )
	, table()
	{
	(void) canceller;
	if( num_waves <= 0 || wavelength <= 0 || int64_t( num_waves ) * wavelength > INT32_MAX ) return;
	if( flanhip_device_count() < 1 ) return;                                     // a table nothing could play: null, like every device-less result
	for( int i = 0; i < num_waves; ++i ) waveform_starts[0][size_t( i )] = i;    // :241-242
	std::vector<float> samples( size_t( num_waves ) * size_t( wavelength ) );
	detail::for_each_index( 0, int( samples.size() ), f.get_execution_policy(), [&]( int x )
		{
		const int waveform = x / wavelength, frame = x % wavelength;
		samples[size_t( x )] = f( waveform + float( frame ) / wavelength );         // :247, into slot `waveform`
		} );
	table = Audio::create_from_buffer( std::move( samples ), 1, 48000 );         // :239
	}

Wavetable::Wavetable()
	: wavelength( 0 )
	, num_source_frames( 0 )
	, waveform_starts()
	, table()
	{
	}

Audio Wavetable::synthesize( Second length, const Function<Second, Frequency> & freq, const Function<Second, float> & ratio, bool smooth,
	Second granularity_time, flan_CANCEL_ARG_CPP ) const
	{
	if( is_null() ) return Audio::create_null();                                 // :275
	AudioBuffer::Format format = table.get_format();                             // :278-280
	format.num_frames = Frame( table.time_to_frame( length ) );
	const Frame granularity = Frame( table.time_to_frame( granularity_time ) ); // :282
	if( format.num_frames < 1 || granularity < 1 )
		{
		std::cerr << "flan: Wavetable::synthesize: a length or a granularity below one frame" << std::endl;
		return Audio::create_null();
		}
	const Frame n = format.num_frames;
	const Channel ch = format.num_channels;
	const float sr = format.sample_rate;

	// freq at every output frame (a block reads the entry of the frame it starts on, :300); a constant is one entry
	std::vector<float> freq_v( freq.is_constant() ? size_t( 1 ) : size_t( n ) );
	if( freq.is_constant() ) freq_v[0] = freq.get_constant();
	else detail::for_each_index( 0, n, freq.get_execution_policy(), [&]( int x ){ freq_v[size_t( x )] = freq( table.frame_to_time( fFrame( x ) ) ); } );
	if( canceller ) return Audio::create_null();

	const int64_t num_blocks = flanhip_wavetable_synth_plan( n, sr, wavelength, granularity, freq_v.data(), int64_t( freq_v.size() ), 0,
		nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr );
	if( num_blocks <= 0 )
		{
		std::cerr << "flan: Wavetable::synthesize refused: " << flanhip_last_error() << std::endl;
		return Audio::create_null();
		}
	std::vector<int64_t> first_out( static_cast<size_t>( num_blocks ) );
	flanhip_wavetable_synth_plan( n, sr, wavelength, granularity, freq_v.data(), int64_t( freq_v.size() ), num_blocks,
		nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, first_out.data(), nullptr, nullptr, nullptr );

	// ratio_to_table_index( ratio( t_b ), channel ) per ( channel, block ) (:301)
	std::vector<float> r( static_cast<size_t>( num_blocks ) ), index( size_t( ch ) * size_t( num_blocks ) );
	if( ratio.is_constant() ) std::fill( r.begin(), r.end(), ratio.get_constant() );
	else detail::for_each_index( 0, int( num_blocks ), ratio.get_execution_policy(), [&]( int b ){ r[size_t( b )] = ratio( table.frame_to_time( fFrame( first_out[size_t( b )] ) ) ); } );
	for( Channel c = 0; c < ch; ++c )
		flanhip_wavetable_table_index( waveform_starts[size_t( c )].data(), int64_t( waveform_starts[size_t( c )].size() ), num_source_frames, r.data(), num_blocks,
			index.data() + size_t( c ) * size_t( num_blocks ) );
	if( canceller ) return Audio::create_null();

	const int64_t slots = table.get_num_frames() / wavelength;
	const size_t ws_bytes = flanhip_wavetable_synth_workspace_bytes( ch, n, sr, wavelength, granularity, freq_v.data(), int64_t( freq_v.size() ) );
	const float * d_table = table.device_data();
	if( !d_table || ws_bytes == 0 ) return Audio::create_null();
	DeviceCall call( "Wavetable::synthesize" );
	float * d_out = call.output<float>( size_t( ch ) * size_t( n ) );
	void * ws = call.workspace( ws_bytes );
	if( !call.ok() ) return Audio::create_null();
	if( !call.launch( flanhip_wavetable_synth_dev( d_table, ch, slots, wavelength, sr, n, granularity, freq_v.data(), int64_t( freq_v.size() ), index.data(),
		num_blocks, smooth ? 1 : 0, d_out, ws, nullptr ) ) ) return Audio::create_null();
	if( call.wait( canceller ) == FLANHIP_ERR_CANCELLED || canceller ) return Audio::create_null();      // :297
	AudioBuffer out = call.finish<AudioBuffer>( format );
	if( out.is_null() ) return Audio::create_null();
	return Audio( std::move( out ) );
	}

int Wavetable::get_num_waveforms( Channel c ) const
	{
	if( c < 0 || size_t( c ) >= waveform_starts.size() ) return 0;
	return int( waveform_starts[size_t( c )].size() );
	}

// One edit of every slot: into a fresh block that the table takes over (the block under the table may be shared)
void Wavetable::edit( int mode, Frame fade_frames )
	{
	if( is_null() ) return;
	const AudioBuffer::Format f = table.get_format();
	const int64_t slots = f.num_frames / wavelength;
	const size_t count = size_t( f.num_channels ) * size_t( f.num_frames );
	if( count % 4 != 0 )
		{
		// flanhip_copy_dev moves 16 bytes per lane: a table it cannot copy is edited through the host form
		detail::report( flanhip_wavetable_edit( table.get_sample_pointer( 0, 0 ), f.num_channels, slots, wavelength, mode, fade_frames, nullptr ), "Wavetable edit" );
		return;
		}
	const float * d_table = table.device_data();
	if( !d_table ) return;
	AudioBuffer out = detail::device_call<AudioBuffer, float>( "Wavetable edit", f, count, true, detail::kNoWorkspace, [&]( float * d_out, void * )
		{
		if( int rc = flanhip_copy_dev( d_table, d_out, int64_t( count ), nullptr ) ) return rc;
		return flanhip_wavetable_edit_dev( d_out, f.num_channels, slots, wavelength, mode, fade_frames, nullptr );
		} );
	if( !out.is_null() ) table = Audio( std::move( out ) );
	}

void Wavetable::add_fades_in_place( Frame fade_frames ) { edit( FLANHIP_WAVETABLE_ADD_FADES, fade_frames ); }
void Wavetable::remove_jumps_in_place( Frame fade_frames ) { edit( FLANHIP_WAVETABLE_REMOVE_JUMPS, fade_frames ); }
void Wavetable::remove_dc_in_place() { edit( FLANHIP_WAVETABLE_REMOVE_DC, 1 ); }
void Wavetable::normalize_in_place() { edit( FLANHIP_WAVETABLE_NORMALIZE, 1 ); }

bool Wavetable::is_null() const                                                  // :490-503
	{
	if( wavelength <= 0 ) return true;
	if( waveform_starts.empty() ) return true;
	for( const auto & w : waveform_starts ) if( w.empty() ) return true;
	if( num_source_frames <= 0 ) return true;
	if( table.is_null() ) return true;
	return false;
	}

} // namespace flan
