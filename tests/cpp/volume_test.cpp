// volume_test.cpp -- Audio::ring_modulate, fade / fade_frames and their in-place forms, invert_phase, waveshape, add_moisture, apply_adsr_envelope,
// apply_ar_envelope, get_total_energy, get_energy_difference, get_amplitude_envelope, synthesize_waveform, synthesize_white_noise, flan::ADSR and
// flan::Waveform (include/flan/Audio.h, include/flan/Function.h) over libflan_host.so.
//   volume_test --no-device          null inputs, what is decided on the host (the ADSR anchors, the named waveforms as host functions, refusals);
//                                    without a device the methods fail loudly with null Audios and empty vectors
//   volume_test --device             what can be said without a second opinion: every method against the composition of public pieces it is
//                                    defined as, bit for bit; seeds; the envelope Function
//   volume_test --dump IN DIR        IN: raw fp32 in [-1, 1], a pool of at least 40100 floats: an Audio of ch x n is its first ch * n floats.  Writes
//                                    every result to DIR/<name>.bin (int32 channels, int32 frames, float sample rate, the samples) for the Python
//                                    suite, which computes the same with tests/volume_reference.py
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "flan/flan.h"
#include "flanhip.h"

using namespace flan;

static int failures = 0;
#define CHECK( cond ) do { if( !( cond ) ) { std::printf( "FAILED: %s (line %d)\n", #cond, __LINE__ ); ++failures; } } while( 0 )

static bool same_bits( const Audio & a, const Audio & b )
	{
	if( a.is_null() || b.is_null() ) return a.is_null() && b.is_null();
	return a.get_num_channels() == b.get_num_channels() && a.get_num_frames() == b.get_num_frames() && a.get_sample_rate() == b.get_sample_rate()
		&& std::memcmp( a.get_buffer().data(), b.get_buffer().data(), sizeof( float ) * a.get_buffer().size() ) == 0;
	}

static std::vector<float> noise( size_t n, uint32_t seed )
	{
	std::vector<float> v( n );
	for( size_t i = 0; i < n; ++i )
		{
		seed = seed * 1664525u + 1013904223u;
		v[i] = float( int32_t( seed >> 8 ) - ( 1 << 23 ) ) / float( 1 << 23 );
		}
	return v;
	}

static Audio noisy( Channel ch, Frame n, uint32_t seed, float sr = 48000.0f )
	{
	return Audio::create_from_buffer( noise( size_t( ch ) * size_t( n ), seed ), ch, sr );
	}

static const auto soft_clip = []( std::pair<Second, Sample> ts ) -> Sample { return ts.second / ( 1.0f + std::abs( ts.second ) ); };
static const auto timed = []( std::pair<Second, Sample> ts ) -> Sample { return ts.second * ( 1.0f - 40.0f * ts.first ); };
static const auto saw_by_hand = []( Second t ) -> Amplitude { const Second t0 = std::fmod( t, 1.0f ); return -1.0f + 2.0f * t0; };
static const auto sine_by_hand = []( Second t ) -> Amplitude { const Second t0 = std::fmod( t, 1.0f ); return std::sin( pi2 * t0 ); };

static void null_checks()
	{
	const Audio none, some = noisy( 1, 10, 1 );
	CHECK( none.ring_modulate( some ).is_null() && some.ring_modulate( none ).is_null() );
	CHECK( none.fade().is_null() && none.fade_frames().is_null() && none.invert_phase().is_null() );
	Audio held;
	CHECK( held.fade_in_place().is_null() && held.fade_frames_in_place().is_null() );
	CHECK( none.waveshape( Function<std::pair<Second, Sample>, Sample>( soft_clip ) ).is_null() && none.add_moisture().is_null() );
	CHECK( none.apply_adsr_envelope( 0.1f, 0.1f, 0.1f, 0.1f, 0.5f ).is_null() && none.apply_ar_envelope( 0.1f, 0.1f ).is_null() );
	CHECK( none.get_total_energy().empty() && none.get_energy_difference( some ).empty() && some.get_energy_difference( none ).empty() );
	const auto zero = none.get_amplitude_envelope();
	CHECK( zero.is_constant() && zero( 0.5f ) == 0.0f );
	}

// what is decided before the device
static void host_checks()
	{
	const Audio a = noisy( 2, 500, 2 );
	CHECK( a.waveshape( Function<std::pair<Second, Sample>, Sample>( soft_clip ), 0 ).is_null() );                  // a sample rate of 0
	const auto flat = a.get_amplitude_envelope( 0.0f ), negative = a.get_amplitude_envelope( -1.0f );
	CHECK( flat.is_constant() && flat( 0.001f ) == 0.0f && negative.is_constant() );
	CHECK( Audio::synthesize_waveform( waveforms::sine, 0.1f, 440.0f, 48000.0f, 0 ).is_null() );                     // AudioSynthesis.cpp:33
	CHECK( Audio::synthesize_waveform( waveforms::sine, 0.0f, 440.0f ).is_null() && Audio::synthesize_waveform( waveforms::sine, -1.0f, 440.0f ).is_null() );
	CHECK( Audio::synthesize_waveform( waveforms::sine, 0.1f, 440.0f, 0.0f ).is_null() && Audio::synthesize_waveform( waveforms::sine, 0.1f, 440.0f, -8.0f ).is_null() );
	CHECK( Audio::synthesize_white_noise( 0.1f, 48000.0f, 0, 1 ).is_null() && Audio::synthesize_white_noise( 0.0f, 48000.0f, 16, 1 ).is_null() );
	CHECK( Audio::synthesize_white_noise( 0.1f, 0.0f, 16, 1 ).is_null() );
	// the named waveforms carry their kinds and are, as host functions, flanhip_waveform_host's; a callable has none
	const Waveform * named[4] = { &waveforms::sine, &waveforms::square, &waveforms::saw, &waveforms::triangle };
	const std::vector<float> t = { 0.0f, 0.25f, 0.5f, 0.75f, 1.0f, 1.3f, -0.25f, -0.5f, -0.75f, -1.3f, 603.18f, -7.77f };
	for( int k = 0; k < 4; ++k )
		{
		CHECK( named[k]->kind() == k );
		std::vector<float> want( t.size() );
		CHECK( flanhip_waveform_host( k, t.data(), int64_t( t.size() ), want.data() ) == FLANHIP_OK );
		for( size_t i = 0; i < t.size(); ++i ) CHECK( ( *named[k] )( t[i] ) == want[i] );
		}
	CHECK( FLANHIP_WAVEFORM_SINE == 0 && FLANHIP_WAVEFORM_SQUARE == 1 && FLANHIP_WAVEFORM_SAW == 2 && FLANHIP_WAVEFORM_TRIANGLE == 3 );
	CHECK( waveforms::square( -0.25f ) == -1.0f && waveforms::saw( -0.25f ) == -1.5f && waveforms::triangle( -0.25f ) == -2.0f );      // fmod keeps the sign
	CHECK( Waveform( saw_by_hand ).kind() == -1 && Waveform( saw_by_hand, ExecutionPolicy::Linear_Sequenced ).get_execution_policy() == ExecutionPolicy::Linear_Sequenced );
	// the ADSR anchors (Function.cpp:23-28), every time exact in fp32
	const auto env = ADSR( 0.5f, 0.25f, 1.0f, 0.25f, 0.5f );
	CHECK( env( -0.001f ) == 0.0f && env( 2.5f ) == 0.0f && env( 0.0f ) == 0.0f && env( 0.25f ) == 0.5f );
	CHECK( env( 0.5f ) == 1.0f && env( 0.625f ) == 0.75f && env( 0.75f ) == 0.5f && env( 1.0f ) == 0.5f );         // t == a: the decay begins; t == a + d: the sustain
	CHECK( env( 1.75f ) == 0.5f && env( 1.875f ) == 0.25f && env( 2.0f ) == 0.0f );                                // t == a + d + s: the release begins; its end is 0
	const auto squared = ADSR( 0.5f, 0.25f, 1.0f, 0.25f, 0.5f, 2.0f, 2.0f, 2.0f );
	CHECK( squared( 0.25f ) == 0.25f && squared( 0.625f ) == 0.625f && squared( 1.875f ) == 0.125f );
	int32_t plan[2];
	CHECK( flanhip_fade_frames_plan( 1000, 700, 700, plan ) == FLANHIP_OK && plan[0] == 500 && plan[1] == 500 );
	}

static void no_device_checks()
	{
	host_checks();
	const Audio a = noisy( 2, 500, 3 );
	float * bogus = reinterpret_cast<float*>( uintptr_t( 1 ) << 41 );
	CHECK( flanhip_audio_ring_modulate_dev( bogus, 2, 500, bogus + ( 1 << 20 ), 1, 7, bogus + 4096, nullptr ) == FLANHIP_ERR_NO_DEVICE );
	CHECK( flanhip_audio_fade_dev( bogus, 2, 500, bogus + ( 1 << 20 ), 5, nullptr, 0, bogus, nullptr ) == FLANHIP_ERR_NO_DEVICE );
	CHECK( flanhip_audio_energy_dev( bogus, 2, 500, bogus + ( 1 << 20 ), bogus + ( 1 << 21 ), nullptr ) == FLANHIP_ERR_NO_DEVICE );
	CHECK( a.ring_modulate( a ).is_null() && a.fade_frames( 16, 16 ).is_null() && a.fade( 0.001f, 0.001f ).is_null() && a.invert_phase().is_null() );
	CHECK( same_bits( a.fade_frames( 0, 0 ), a ) && same_bits( a.fade_frames( -5, -5 ), a ) );                        // AudioVolume.cpp:119: nothing to do is a copy
	Audio held = a.copy();
	CHECK( same_bits( held.fade_frames_in_place( 16, 16 ), a ) );                                                    // what could not be computed leaves *this
	CHECK( a.waveshape( Function<std::pair<Second, Sample>, Sample>( soft_clip ) ).is_null() && a.add_moisture().is_null() );
	CHECK( a.add_moisture( .5f, 96, 4, Waveform( sine_by_hand ) ).is_null() );
	CHECK( a.apply_adsr_envelope( 0.001f, 0.001f, 0.001f, 0.001f, 0.5f ).is_null() && a.apply_ar_envelope( 0.001f, 0.001f ).is_null() );
	CHECK( a.get_total_energy().empty() && a.get_energy_difference( a ).empty() );
	const auto env = a.get_amplitude_envelope( 0.001f );
	CHECK( env.is_constant() && env( 0.001f ) == 0.0f );
	CHECK( Audio::synthesize_waveform( waveforms::saw, 0.01f, 440.0f ).is_null() && Audio::synthesize_waveform( Waveform( saw_by_hand ), 0.01f, 440.0f ).is_null() );
	CHECK( Audio::synthesize_white_noise( 0.01f, 48000.0f, 4, 1 ).is_null() );
	}

// a block on the device for the stage-by-stage compositions
struct Dev
	{
	void * p = nullptr;
	explicit Dev( size_t bytes ) { if( flanhip_malloc( &p, bytes ? bytes : 1 ) != FLANHIP_OK ) p = nullptr; }
	~Dev() { if( p ) flanhip_free( p ); }
	float * f() const { return static_cast<float*>( p ); }
	};

static Audio waveshape_by_hand( const Audio & a, const Function<std::pair<Second, Sample>, Sample> & shaper, uint16_t factor )
	{
	Audio over = a.resample( a.get_sample_rate() * factor );
	if( over.is_null() ) return Audio();
	for( Channel c = 0; c < over.get_num_channels(); ++c )
		for( Frame f = 0; f < over.get_num_frames(); ++f )
			over.set_sample( c, f, shaper( std::pair<Second, Sample>( over.frame_to_time( f ), over.get_sample( c, f ) ) ) );
	return over.resample( a.get_sample_rate() );
	}

// up-chain, flanhip_audio_moisture_dev, down-chain, each through its own entry point
static Audio moisture_by_stages( const Audio & a, float amount, float frequency, float skew, int kind )
	{
	const Audio over = a.resample( a.get_sample_rate() * 4 );
	if( over.is_null() ) return Audio();
	const size_t count = size_t( over.get_num_channels() ) * size_t( over.get_num_frames() );
	Dev shaped( sizeof( float ) * count );
	std::vector<float> host( count );
	if( !shaped.p || flanhip_audio_moisture_dev( over.device_data(), over.get_num_channels(), over.get_num_frames(), over.get_sample_rate(), a.get_num_frames(),
		a.get_sample_rate(), nullptr, amount, nullptr, frequency, nullptr, skew, kind, shaped.f(), nullptr ) != FLANHIP_OK ) return Audio();
	if( flanhip_stream_synchronize( nullptr ) != FLANHIP_OK || flanhip_download( host.data(), shaped.p, sizeof( float ) * count ) != FLANHIP_OK ) return Audio();
	return Audio::create_from_buffer( std::move( host ), over.get_num_channels(), over.get_sample_rate() ).resample( a.get_sample_rate() );
	}

// the scan with the waveform in its replay, then the chain with the explicit length, each through its own entry point; wave_out: the wave samples
static Audio oscillator_by_stages( int kind, const std::vector<float> * freq, float freq_c, float length, float sr, int oversample, std::vector<float> * wave_out = nullptr )
	{
	int64_t n_in = 0; double in_rate = 0;
	const int64_t n = flanhip_synthesize_waveform_frames( length, sr, oversample, &n_in, &in_rate );
	if( n <= 0 ) return Audio();
	Dev d_freq( sizeof( float ) * size_t( n_in ) ), d_wave( sizeof( float ) * size_t( n_in ) ), d_out( sizeof( float ) * size_t( n ) ), d_ws( flanhip_osc_workspace_bytes( n_in ) );
	if( !d_freq.p || !d_wave.p || !d_out.p || !d_ws.p ) return Audio();
	if( freq && flanhip_upload( d_freq.p, freq->data(), sizeof( float ) * size_t( n_in ) ) != FLANHIP_OK ) return Audio();
	if( flanhip_osc_phase_dev( freq ? d_freq.f() : nullptr, freq_c, n_in, in_rate, nullptr, d_wave.f(), kind, d_ws.p, nullptr ) != FLANHIP_OK ) return Audio();
	if( flanhip_oneshot_resample_dev( d_wave.f(), n_in, in_rate, double( sr ), d_out.f(), n, nullptr ) != FLANHIP_OK ) return Audio();
	std::vector<float> host( static_cast<size_t>( n ) );
	if( flanhip_stream_synchronize( nullptr ) != FLANHIP_OK || flanhip_download( host.data(), d_out.p, sizeof( float ) * size_t( n ) ) != FLANHIP_OK ) return Audio();
	if( wave_out ) { wave_out->resize( size_t( n_in ) ); if( flanhip_download( wave_out->data(), d_wave.p, sizeof( float ) * size_t( n_in ) ) != FLANHIP_OK ) return Audio(); }
	return Audio::create_from_buffer( std::move( host ), 1, sr );
	}

static void device_checks()
	{
	host_checks();
	// ---- ring_modulate: a modulator longer than the input reads its beginning; 1 x 1
	{
	const Audio a = noisy( 2, 100, 4 ), longer = noisy( 1, 250, 5 ), one = noisy( 1, 1, 6 );
	const Audio r = a.ring_modulate( longer );
	CHECK( !r.is_null() && r.get_sample( 1, 99 ) == a.get_sample( 1, 99 ) * longer.get_sample( 0, 99 ) && r.get_sample( 0, 0 ) == a.get_sample( 0, 0 ) * longer.get_sample( 0, 0 ) );
	const Audio sq = one.ring_modulate( one );
	CHECK( sq.get_num_frames() == 1 && sq.get_sample( 0, 0 ) == one.get_sample( 0, 0 ) * one.get_sample( 0, 0 ) );
	}
	// ---- invert_phase: the sign bit and nothing else, specials included
	{
	Audio a = noisy( 2, 1003, 7 );
	a.set_sample( 0, 0, 0.0f ); a.set_sample( 0, 1, -0.0f ); a.set_sample( 0, 2, 1e-41f ); a.set_sample( 1, 1002, INFINITY ); a.set_sample( 1, 5, -INFINITY );
	const Audio inv = a.invert_phase();
	bool flipped = !inv.is_null();
	for( size_t i = 0; flipped && i < a.get_buffer().size(); ++i )
		{
		uint32_t x, y;
		std::memcpy( &x, &a.get_buffer()[i], 4 ); std::memcpy( &y, &inv.get_buffer()[i], 4 );
		flipped = y == ( x ^ 0x80000000u );
		}
	CHECK( flipped && same_bits( inv.invert_phase(), a ) );
	}
	// ---- the fades: seconds are frames; nothing to do is a copy; the in-place forms take the result over
	{
	const Audio a = noisy( 2, 1000, 8 );
	CHECK( same_bits( a.fade( 0.01f, 0.002f ), a.fade_frames( Frame( a.time_to_frame( 0.01f ) ), Frame( a.time_to_frame( 0.002f ) ) ) ) );
	CHECK( same_bits( a.fade(), a.fade_frames( 16, 16, Interpolator::sqrt() ) ) && same_bits( a.fade_frames(), a.fade_frames( 16, 16 ) ) );
	CHECK( same_bits( a.fade_frames( 0, 0 ), a ) && same_bits( a.fade_frames( -4, -9 ), a ) && same_bits( a.fade_frames( -4, 7 ), a.fade_frames( 0, 7 ) ) );
	const Audio f = a.fade_frames( 16, 16 );
	CHECK( f.get_sample( 0, 0 ) == 0.0f && f.get_sample( 1, 999 ) == 0.0f && f.get_sample( 0, 500 ) == a.get_sample( 0, 500 ) && f.get_sample( 1, 4 ) == a.get_sample( 1, 4 ) * std::sqrt( 4.0f / 16 ) );
	Audio held = a.copy();
	CHECK( same_bits( held.fade_frames_in_place( 30, 40, Interpolator::linear() ), a.fade_frames( 30, 40, Interpolator::linear() ) ) );
	Audio timed_held = a.copy();
	CHECK( same_bits( timed_held.fade_in_place( 0.003f, 0.001f ), a.fade( 0.003f, 0.001f ) ) );
	CHECK( same_bits( a.fade_frames( 700, 700, Interpolator::linear() ), a.fade_frames( 500, 500, Interpolator::linear() ) ) );       // the shrink
	}
	// ---- waveshape: the composition of the public pieces, bit for bit
	for( uint16_t factor : { uint16_t( 4 ), uint16_t( 3 ) } )
		for( const auto & shape : { std::pair<Channel, Frame>( 3, 777 ), std::pair<Channel, Frame>( 1, 50 ) } )
			{
			const Audio a = noisy( shape.first, shape.second, 9 + factor );
			const Function<std::pair<Second, Sample>, Sample> clip( soft_clip ), by_time( timed, ExecutionPolicy::Linear_Sequenced );
			const Audio got = a.waveshape( clip, factor );
			CHECK( !got.is_null() && got.get_num_frames() == a.get_num_frames() && same_bits( got, waveshape_by_hand( a, clip, factor ) ) );
			CHECK( same_bits( a.waveshape( by_time, factor ), waveshape_by_hand( a, by_time, factor ) ) );
			}
	// ---- add_moisture: the defaults are the named sine on the device; it is the three stages; another waveform is waveshape on the host
	for( const auto & shape : { std::pair<Channel, Frame>( 2, 20001 ), std::pair<Channel, Frame>( 1, 50 ) } )
		{
		const Audio a = noisy( shape.first, shape.second, 21 );
		const Audio wet = a.add_moisture();
		CHECK( !wet.is_null() && wet.get_num_frames() == a.get_num_frames() && wet.get_num_channels() == a.get_num_channels() );
		CHECK( same_bits( wet, a.add_moisture( .5f, 96, 4, waveforms::sine ) ) && same_bits( wet, moisture_by_stages( a, 0.5f, 96.0f, 4.0f, FLANHIP_WAVEFORM_SINE ) ) );
		CHECK( same_bits( a.add_moisture( 0.25f, 3.0f, 2.0f, waveforms::triangle ), moisture_by_stages( a, 0.25f, 3.0f, 2.0f, FLANHIP_WAVEFORM_TRIANGLE ) ) );
		// constants and curves that return them give the same bits: a curve is read, a scalar is passed
		const Function<Second, float> amount( []( Second ){ return 0.5f; } ), frequency( []( Second ){ return 96.0f; } ), skew( []( Second ){ return 4.0f; } );
		CHECK( same_bits( wet, a.add_moisture( amount, frequency, skew ) ) );
		if( shape.second == 50 )
			{
			const Function<std::pair<Second, Sample>, Sample> shaper( [&a]( std::pair<Second, Sample> ts ) -> Sample
				{
				const float power = ts.second >= 0 ? std::pow( ts.second, 4.0f ) : -std::pow( -ts.second, 4.0f );
				return ts.second + 0.5f * ts.second * sine_by_hand( pi2 * 96.0f * power );
				} );
			CHECK( same_bits( a.add_moisture( .5f, 96, 4, Waveform( sine_by_hand ) ), waveshape_by_hand( a, shaper, 4 ) ) );
			}
		}
	// ---- synthesize_waveform: the scan, the waveform and the chain with the explicit length, nothing added; a callable takes the host's way
	{
	std::vector<float> wave;
	const Audio saw = Audio::synthesize_waveform( waveforms::saw, 0.05f, 440.0f, 48000.0f, 16 );
	CHECK( !saw.is_null() && saw.get_num_channels() == 1 && saw.get_num_frames() == 2400 && saw.get_sample_rate() == 48000.0f );
	CHECK( same_bits( saw, oscillator_by_stages( FLANHIP_WAVEFORM_SAW, nullptr, 440.0f, 0.05f, 48000.0f, 16 ) ) );
	CHECK( same_bits( saw, Audio::synthesize_waveform( Waveform( saw_by_hand ), 0.05f, 440.0f, 48000.0f, 16 ) ) );      // the same fp32 expression at the same phases
	const Function<Second, Frequency> sweep( []( Second t ){ return 200.0f + 9000.0f * t; } );
	int64_t n_in = 0; double in_rate = 0;
	CHECK( flanhip_synthesize_waveform_frames( 0.031f, 44100.0f, 3, &n_in, &in_rate ) == 1367 && n_in == 4101 );
	std::vector<float> curve( static_cast<size_t>( n_in ) );
	for( int64_t i = 0; i < n_in; ++i ) curve[size_t( i )] = sweep( Second( int( i ) * float( 1.0f / in_rate ) ) );
	CHECK( same_bits( Audio::synthesize_waveform( waveforms::sine, 0.031f, sweep, 44100.0f, 3 ), oscillator_by_stages( FLANHIP_WAVEFORM_SINE, &curve, 0, 0.031f, 44100.0f, 3 ) ) );
	// oversample 1: equal rates: the wave samples themselves (CDSPResampler.h:133-136)
	const Audio direct = Audio::synthesize_waveform( waveforms::triangle, 0.01f, 1000.0f, 48000.0f, 1 );
	const Audio staged = oscillator_by_stages( FLANHIP_WAVEFORM_TRIANGLE, nullptr, 1000.0f, 0.01f, 48000.0f, 1, &wave );
	CHECK( direct.get_num_frames() == 480 && same_bits( direct, staged ) && wave.size() == 480 && !std::memcmp( wave.data(), direct.get_buffer().data(), 480 * sizeof( float ) ) );
	CHECK( direct.get_sample( 0, 0 ) == -1.0f );                                                                       // phase 0
	}
	// ---- synthesize_white_noise: the host draw, then resample; a seed names one result
	{
	const Audio w = Audio::synthesize_white_noise( 0.02f, 48000.0f, 4, 77 );
	CHECK( !w.is_null() && w.get_num_frames() == 960 && same_bits( w, Audio::synthesize_white_noise( 0.02f, 48000.0f, 4, 77 ) ) );
	CHECK( !same_bits( w, Audio::synthesize_white_noise( 0.02f, 48000.0f, 4, 78 ) ) );
	Audio drawn = Audio::create_empty_with_length( 0.02f, 1, 48000.0f * 4 );
	CHECK( flanhip_white_noise_draw( 77, drawn.get_num_frames(), drawn.get_buffer().data() ) == FLANHIP_OK );
	CHECK( same_bits( w, drawn.resample( 48000.0f ) ) );
	const Audio same_rate = Audio::synthesize_white_noise( 0.001f, 48000.0f, 1, 5 );                                    // oversample 1: resample is a copy
	CHECK( same_rate.get_num_frames() == 48 && same_rate.get_sample( 0, 0 ) >= -1.0f && same_rate.get_sample( 0, 0 ) <= 1.0f );
	}
	// ---- the envelopes are modify_volume of the ADSR
	{
	const Audio a = noisy( 2, 4800, 31 );
	CHECK( same_bits( a.apply_adsr_envelope( 0.02f, 0.01f, 0.03f, 0.02f, 0.4f, 2.0f, 0.5f, 3.0f ), a.modify_volume( ADSR( 0.02f, 0.01f, 0.03f, 0.02f, 0.4f, 2.0f, 0.5f, 3.0f ) ) ) );
	CHECK( same_bits( a.apply_ar_envelope( 0.03f, 0.05f, 2.0f, 0.5f ), a.modify_volume( ADSR( 0.03f, 0, 0, 0.05f, 1, 2.0f, 1, 0.5f ) ) ) );
	CHECK( a.apply_ar_envelope( 0.03f, 0.05f ).get_sample( 1, 4799 ) == 0.0f );                                        // past the release
	}
	// ---- the energies
	{
	const Audio a = noisy( 3, 100003, 41 );
	const std::vector<float> e = a.get_total_energy();
	CHECK( e.size() == 3 && e == a.get_total_energy() && e[0] > 30000.0f && e[0] < 36000.0f );                         // uniform in [-1, 1): n / 3
	const std::vector<float> none = a.get_energy_difference( a );
	CHECK( none.size() == 3 && none[0] == 0.0f && none[1] == 0.0f && none[2] == 0.0f );
	const Audio half = a.modify_volume( 0.5f );
	CHECK( a.get_energy_difference( half ) == half.get_total_energy() );                                               // x - 0.5 x is 0.5 x exactly
	const Audio other_rate = Audio::create_from_buffer( std::vector<float>( a.get_buffer().begin(), a.get_buffer().begin() + 3 * 2000 ), 3, 96000.0f );
	const Audio short_a = Audio::create_from_buffer( std::vector<float>( a.get_buffer().begin(), a.get_buffer().begin() + 3 * 1000 ), 3, 48000.0f );
	const std::vector<float> across = short_a.get_energy_difference( other_rate );
	const Audio at_this_rate = other_rate.resample( 48000.0f );                                                       // AudioInformation.cpp:133: the other comes to this rate
	CHECK( across.size() == 3 && across == Audio::mix( std::vector<const Audio *>{ &short_a, &at_this_rate }, { 0, 0 }, { 1, -1 } ).get_total_energy() && across[0] > 0.0f );
	}
	// ---- get_amplitude_envelope: the composition through the public pieces and the rectifier's entry point, then the Function's own arithmetic
	{
	const Audio a = noisy( 2, 3000, 51 );
	const auto env = a.get_amplitude_envelope( 0.01f );
	const Audio mono = a.convert_to_mono();
	Dev rect( sizeof( float ) * 3000 );
	std::vector<float> host( 3000 );
	CHECK( rect.p && flanhip_audio_rectify_dev( mono.device_data(), 1, 3000, rect.f(), nullptr ) == FLANHIP_OK && flanhip_stream_synchronize( nullptr ) == FLANHIP_OK
		&& flanhip_download( host.data(), rect.p, sizeof( float ) * 3000 ) == FLANHIP_OK );
	for( Frame f = 0; f < 3000; ++f ) CHECK( host[size_t( f )] == std::abs( mono.get_sample( 0, f ) ) );
	std::vector<float> window( 480 );
	float total = 0;
	for( int i = 0; i < 480; ++i ) { window[size_t( i )] = float( 0.5 * ( 1.0 - std::cos( double( 2.0f * pi * ( float( i ) / ( 480.0f - 1 ) ) ) ) ) ); total += window[size_t( i )]; }
	Audio ys = Audio::create_from_buffer( std::move( host ), 1, 48000.0f ).convolve( Audio::create_from_buffer( std::move( window ), 1, 48000.0f ), false );
	ys.modify_volume_in_place( pi / 2.0f / total );
	CHECK( ys.get_num_frames() == 3480 );
	bool linear = !env.is_constant();
	for( Frame f = 0; linear && f < 3479; f += 7 )
		{
		const float t = ( f + 0.5f ) / 48000.0f, x = t * 48000.0f;                                                      // a frame's mid-point
		const Frame x1 = Frame( std::floor( x ) );
		linear = env( t ) == ys.get_sample( 0, x1 ) + ( ys.get_sample( 0, x1 + 1 ) - ys.get_sample( 0, x1 ) ) * ( x - x1 );
		}
	CHECK( linear && env( 0.0f ) == ys.get_sample( 0, 0 ) && env( -0.0001f ) == 0.0f && env( 3479.0f / 48000.0f ) == 0.0f && env( 1.0f ) == 0.0f );
	CHECK( env( 1500.5f / 48000.0f ) > 0.3f && env( 1500.5f / 48000.0f ) < 0.7f );                                     // the mean of |uniform mono| is near 1 / 3, times pi / 2
	}
	std::printf( "volume methods on the device\n" );
	}

static bool write_audio( const std::string & dir, const std::string & name, const Audio & a )
	{
	std::FILE * out = std::fopen( ( dir + "/" + name + ".bin" ).c_str(), "wb" );
	if( !out ) { std::printf( "FAILED: cannot write %s\n", name.c_str() ); return false; }
	const int32_t shape[2] = { a.is_null() ? 0 : a.get_num_channels(), a.is_null() ? 0 : a.get_num_frames() };
	const float sr = a.is_null() ? 0.0f : a.get_sample_rate();
	std::fwrite( shape, sizeof( int32_t ), 2, out );
	std::fwrite( &sr, sizeof( float ), 1, out );
	if( !a.is_null() ) std::fwrite( a.get_buffer().data(), sizeof( float ), a.get_buffer().size(), out );
	std::fclose( out );
	return true;
	}

static int dump( const char * in_path, const std::string & dir )
	{
	std::FILE * in = std::fopen( in_path, "rb" );
	if( !in ) { std::printf( "FAILED: cannot read %s\n", in_path ); return 1; }
	std::vector<float> x;
	float block[4096];
	for( size_t got; ( got = std::fread( block, sizeof( float ), 4096, in ) ) > 0; ) x.insert( x.end(), block, block + got );
	std::fclose( in );
	if( x.size() < 40100 ) { std::printf( "FAILED: the pool is too small\n" ); return 1; }
	const auto take = [&]( Channel ch, Frame n, float sr = 48000.0f ) { return Audio::create_from_buffer( std::vector<float>( x.begin(), x.begin() + size_t( ch ) * size_t( n ) ), ch, sr ); };
	bool ok = true;
	const auto put = [&]( const std::string & name, const Audio & a ){ ok = write_audio( dir, name, a ) && ok; };

	const Audio A = take( 2, 1000 );
	const Interpolator squared( []( float v ){ return v * v; } );
	const Interpolator * interps[3] = { nullptr, nullptr, &squared };
	const Interpolator root = Interpolator::sqrt(), line = Interpolator::linear();
	interps[0] = &root; interps[1] = &line;
	const char * names[3] = { "sqrt", "linear", "callable" };
	const int cases[6][2] = { { 16, 16 }, { 0, 7 }, { 7, 0 }, { 0, 0 }, { 700, 700 }, { -3, -4 } };
	for( int k = 0; k < 3; ++k )
		for( const auto & c : cases )
			put( std::string( "fade_" ) + names[k] + "_" + std::to_string( c[0] ) + "_" + std::to_string( c[1] ), A.fade_frames( c[0], c[1], *interps[k] ) );
	put( "fade_rows_333", take( 3, 333 ).fade_frames( 50, 21 ) );                     // rows 1 and 2 start off a 16-byte boundary
	put( "fade_seconds", A.fade( 0.004f, 0.0015f, line ) );
	put( "ring", take( 3, 1001 ).ring_modulate( take( 2, 37 ) ) );
	put( "invert", A.invert_phase() );
	// a sample rate of 16: every frame time and every segment boundary of the envelope is exact in fp32
	const Audio slow = take( 2, 64, 16.0f );
	put( "adsr", slow.apply_adsr_envelope( 0.5f, 0.25f, 1.0f, 0.25f, 0.5f ) );                 // exponents of 1: pow( x, 1 ) is x in every library
	put( "ar", slow.apply_ar_envelope( 0.5f, 1.5f ) );
	put( "adsr_48k", A.apply_adsr_envelope( 0.004f, 0.003f, 0.005f, 0.006f, 0.3f, 1.5f, 2.0f, 0.7f ) );
	put( "moisture_2x20001", take( 2, 20001 ).add_moisture() );
	put( "moisture_1x50", take( 1, 50 ).add_moisture() );
	put( "moisture_low", take( 2, 20001 ).add_moisture( 0.5f, 3.0f, 4.0f ) );
	const Function<Second, float> amount( []( Second t ){ return 0.2f + t; } ), frequency( []( Second t ){ return 40.0f + 100.0f * t; } ), skew( []( Second t ){ return 2.0f + 3.0f * t; } );
	put( "moisture_curves", take( 2, 20001 ).add_moisture( amount, frequency, skew ) );
	const Audio E = take( 3, 4099 );
	{
	std::vector<float> e = E.get_total_energy(), d = E.get_energy_difference( E.modify_volume( 0.5f ) );
	if( e.size() != 3 || d.size() != 3 ) { std::printf( "FAILED: the energies\n" ); ok = false; }
	else { put( "energy", Audio::create_from_buffer( std::move( e ), 1, 1.0f ) ); put( "energy_half", Audio::create_from_buffer( std::move( d ), 1, 1.0f ) ); }
	}
	{
	// frame f's time f / 48000 is not always exact; at a rate of 65536 it is, and there the Function returns its own samples: ys[f] for
	// f < size - 1, 0 from there on
	std::vector<float> ys( 3480 + 2 );
	const auto env_exact = take( 2, 3000, 65536.0f ).get_amplitude_envelope( 480.0f / 65536.0f );
	for( int f = 0; f < 3482; ++f ) ys[size_t( f )] = env_exact( float( f ) / 65536.0f );
	put( "envelope", Audio::create_from_buffer( std::move( ys ), 1, 65536.0f ) );
	}
	put( "osc_saw", Audio::synthesize_waveform( waveforms::saw, 0.05f, 440.0f, 48000.0f, 16 ) );
	put( "noise_77", Audio::synthesize_white_noise( 0.02f, 48000.0f, 4, 77 ) );
	return ok ? 0 : 1;
	}

int main( int argc, char ** argv )
	{
	const char * mode = argc > 1 ? argv[1] : "--no-device";
	std::ostringstream captured;                                               // "Null Audio created"
	std::streambuf * old = std::cout.rdbuf( captured.rdbuf() );
	null_checks();
	if( !std::strcmp( mode, "--no-device" ) ) no_device_checks();
	if( !std::strcmp( mode, "--device" ) || !std::strcmp( mode, "--dump" ) )
		{
		if( flanhip_device_count() < 1 ) { std::cout.rdbuf( old ); std::printf( "FAILED: no device\n" ); return 1; }
		if( !std::strcmp( mode, "--device" ) ) device_checks();
		else if( argc < 4 || dump( argv[2], argv[3] ) ) ++failures;
		}
	std::cout.rdbuf( old );
	std::printf( failures ? "%d FAILED\n" : "PASSED\n", failures );
	return failures ? 1 : 0;
	}
