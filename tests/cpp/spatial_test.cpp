// spatial_test.cpp -- Audio::stereo_spatialize, pan / pan_in_place / widen, convert_to_stereo / convert_to_mono, combine_channels /
// split_channels (include/flan/Audio.h) over libflan_host.so.
//   spatial_test --no-device  null in, null out; a non-mono input of stereo_spatialize is refused with the reference's message; without a
//                             device the C ABI answers FLANHIP_ERR_NO_DEVICE and the methods fail loudly with a null result, nothing sampled
//   spatial_test --device     stereo_spatialize with a constant position (the pure delay, its length included) and with a callable orbit
//                             against the C ABI fed what the method samples, bit for bit; a moving source on 32 frames or fewer gives a null
//                             Audio and one line; pan, widen, the conversions and the channel copies against host loops, bit for bit
//   spatial_test --bench S    the whole method on S seconds of audio, timed (tools/bench_spatial.py)
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <iostream>
#include <limits>
#include <sstream>
#include <vector>

#include "flan/flan.h"
#include "flanhip.h"

using namespace flan;

static int failures = 0;
#define CHECK( cond ) do { if( !( cond ) ) { std::printf( "FAILED: %s (line %d)\n", #cond, __LINE__ ); ++failures; } } while( 0 )

static bool same_bits( const void * a, const void * b, size_t bytes ) { return std::memcmp( a, b, bytes ) == 0; }
static bool same_audio( const Audio & a, const std::vector<float> & want )
	{
	return !a.is_null() && a.get_buffer().size() == want.size() && same_bits( a.get_buffer().data(), want.data(), sizeof( float ) * want.size() );
	}

static std::vector<float> noise( size_t n, uint32_t seed )
	{
	std::vector<float> v( n );
	for( size_t i = 0; i < n; ++i ) { seed = seed * 1664525u + 1013904223u; v[i] = float( int32_t( seed >> 8 ) - ( 1 << 23 ) ) / float( 1 << 24 ); }
	return v;
	}

static const auto orbit = []( Second t ){ return vec2( 2.0f * std::cos( 31.0f * t ), 0.5f + 2.0f * std::sin( 31.0f * t ) ); };    // 62 m/s
static const auto sway = []( Second t ){ return 0.9f * std::sin( 40.0f * t ); };

// what needs no device
static void refusal_checks()
	{
	std::ostringstream captured, errors;
	std::streambuf * old = std::cout.rdbuf( captured.rdbuf() ), * old_err = std::cerr.rdbuf( errors.rdbuf() );
	int sampled = 0;
	const Function<Second, vec2> counted( [&]( Second ){ ++sampled; return vec2( 1, 1 ); }, ExecutionPolicy::Linear_Sequenced );
	const Function<Second, float> counted_pan( [&]( Second ){ ++sampled; return 0.5f; }, ExecutionPolicy::Linear_Sequenced );
	CHECK( Audio().pan( counted_pan ).is_null() );
	CHECK( Audio().widen( counted_pan ).is_null() );
	CHECK( Audio().convert_to_stereo().is_null() );
	CHECK( Audio().convert_to_mono().is_null() );
	CHECK( Audio().split_channels().empty() );
	CHECK( Audio::combine_channels( std::vector<const Audio *>() ).is_null() );
	CHECK( Audio::combine_channels( std::vector<Audio>() ).is_null() );
	Audio nothing;
	CHECK( nothing.pan_in_place( counted_pan ).is_null() );
	CHECK( captured.str().find( "Null input" ) != std::string::npos );
	CHECK( captured.str().find( "only operates on mono" ) == std::string::npos );
	// stereo_spatialize: anything but mono, a null Audio included, is refused with the reference's words
	CHECK( Audio().stereo_spatialize( counted ).is_null() );
	CHECK( captured.str().find( "Audio::spacialize only operates on mono inputs." ) != std::string::npos );
	captured.str( "" );
	const Audio stereo = Audio::create_from_buffer( noise( 2 * 500, 3 ), 2, 48000.0f );
	CHECK( stereo.stereo_spatialize( counted, 0.18f, counted_pan ).is_null() );
	CHECK( captured.str().find( "Audio::spacialize only operates on mono inputs." ) != std::string::npos );
	// more than two channels cannot be panned; a null among the inputs of combine_channels gives null
	const Audio three = Audio::create_from_buffer( noise( 3 * 100, 4 ), 3, 48000.0f );
	CHECK( three.pan( counted_pan ).is_null() );
	Audio kept = Audio::create_from_buffer( noise( 3 * 100, 4 ), 3, 48000.0f );
	CHECK( kept.pan_in_place( counted_pan ).get_num_channels() == 3 && same_bits( kept.get_buffer().data(), three.get_buffer().data(), sizeof( float ) * 300 ) );
	CHECK( Audio::combine_channels( three, nothing ).is_null() );
	// a moving source on 32 frames or fewer: the reference's zero-frame Audio is a null Audio here, said in one line, nothing sampled
	captured.str( "" );
	const Audio tiny = Audio::create_from_buffer( noise( 32, 5 ), 1, 48000.0f );
	CHECK( tiny.stereo_spatialize( counted ).is_null() );
	CHECK( captured.str().find( "more than 32 frames" ) != std::string::npos );
	std::cout.rdbuf( old ); std::cerr.rdbuf( old_err );
	CHECK( sampled == 0 );
	CHECK( errors.str().empty() );                                             // refusals of the reference's own: nothing on stderr
	}

static void no_device_checks()
	{
	void * bogus = reinterpret_cast<void*>( uintptr_t( 1 ) << 40 );           // never dereferenced
	const float * p = static_cast<const float*>( bogus );
	float * q = static_cast<float*>( bogus ) + 4096;
	const std::vector<double> stretches( 32, 1.0 );
	const int64_t out_frames[2] = { 1100, 1100 };
	const float delays[2] = { 10.0f, 20.0f };
	CHECK( flanhip_spatial_ear_dev( p, p, 1, 1000, 48000.0f, nullptr, 1.0, 1.0, 0.18f, FLANHIP_SPATIAL_BOTH, q, nullptr ) == FLANHIP_ERR_NO_DEVICE );
	CHECK( flanhip_spatial_itd_dev( p, 1, 1000, 48000.0f, stretches.data(), 32, out_frames, 1100, q, bogus, nullptr ) == FLANHIP_ERR_NO_DEVICE );
	CHECK( flanhip_spatial_delay_dev( p, 2, 1000, delays, out_frames, 1100, q, nullptr ) == FLANHIP_ERR_NO_DEVICE );
	CHECK( flanhip_audio_pan_dev( p, 2, 1000, nullptr, 0.5f, q, nullptr ) == FLANHIP_ERR_NO_DEVICE );
	CHECK( flanhip_audio_to_stereo_dev( p, 1000, q, nullptr ) == FLANHIP_ERR_NO_DEVICE );
	CHECK( flanhip_audio_to_mono_dev( p, 2, 1000, q, nullptr ) == FLANHIP_ERR_NO_DEVICE );
	CHECK( flanhip_audio_copy_rows_dev( p, 1000, 2, 1000, q, 1000, 1000, nullptr ) == FLANHIP_ERR_NO_DEVICE );
	const std::vector<float> x = noise( 1000, 1 );
	std::vector<float> out( 2 * x.size() );
	CHECK( flanhip_spatial_ear( x.data(), x.data(), 1, 1000, 48000.0f, nullptr, 1.0, 1.0, 0.18f, FLANHIP_SPATIAL_BOTH, out.data(), nullptr ) == FLANHIP_ERR_NO_DEVICE );
	const Audio a = Audio::create_from_buffer( std::vector<float>( x ), 1, 48000.0f );
	const Audio s = Audio::create_from_buffer( noise( 2 * 1000, 2 ), 2, 48000.0f );
	std::ostringstream captured;
	std::streambuf * old = std::cout.rdbuf( captured.rdbuf() );
	int sampled = 0;
	const Function<Second, vec2> counted( [&]( Second t ){ ++sampled; return orbit( t ); }, ExecutionPolicy::Linear_Sequenced );
	const Function<Second, float> counted_pan( [&]( Second ){ ++sampled; return 0.5f; }, ExecutionPolicy::Linear_Sequenced );
	CHECK( a.stereo_spatialize( vec2( 2, 1 ) ).is_null() );
	CHECK( a.stereo_spatialize( counted, 0.18f, counted_pan ).is_null() );
	CHECK( a.pan( counted_pan ).is_null() );
	CHECK( s.pan( counted_pan ).is_null() );
	CHECK( s.widen( counted_pan ).is_null() );
	CHECK( a.convert_to_stereo().is_null() );
	CHECK( s.convert_to_mono().is_null() );
	CHECK( Audio::combine_channels( a, s ).is_null() );
	const std::vector<Audio> parts = s.split_channels();
	CHECK( parts.size() == 2 && parts[0].is_null() && parts[1].is_null() );
	std::cout.rdbuf( old );
	CHECK( sampled == 0 );                                                     // without a device nothing is sampled
	CHECK( !a.is_null() && same_bits( a.get_buffer().data(), x.data(), sizeof( float ) * x.size() ) );
	}

// the speed limiter of Audio/AudioSpatial.cpp:238-257 over sampled positions, as the method runs it
static void limit( std::vector<double> & ps, const std::vector<float> & speed_limit, float sr )
	{
	for( size_t f = 1; f < ps.size() / 2; ++f )
		{
		const vec2d previous( ps[2 * f - 2], ps[2 * f - 1] );
		const vec2d movement = vec2d( ps[2 * f], ps[2 * f + 1] ) - previous;
		const Meter mag = movement.mag();
		const float c = std::clamp( speed_limit[f], 0.0f, 343.0f - 1.0f ) / sr;
		if( mag > c ) { const vec2d l = previous + movement / mag * c; ps[2 * f] = l.x(); ps[2 * f + 1] = l.y(); }
		}
	}

// stereo_spatialize of a moving source through the C ABI's host forms, from the positions the method samples
static std::vector<float> spatialized( const std::vector<float> & x, float sr, std::vector<double> ps, const std::vector<float> & speed_limit, float head_width, Frame * frames )
	{
	const int64_t n = int64_t( x.size() ), count = ( n + 31 ) / 32;
	limit( ps, speed_limit, sr );
	std::vector<float> lp( x.size() ), shaped( 2 * x.size() );
	CHECK( flanhip_filter_1pole( x.data(), 1, n, sr, nullptr, 500.0f, FLANHIP_FILTER_BUTTERWORTH_LOW, 1, lp.data(), nullptr ) == FLANHIP_OK );
	CHECK( flanhip_spatial_ear( x.data(), lp.data(), 1, n, sr, ps.data(), 0.0, 0.0, head_width, FLANHIP_SPATIAL_BOTH, shaped.data(), nullptr ) == FLANHIP_OK );
	const size_t chunks = size_t( count );
	std::vector<double> dist( chunks ), stretches( 2 * chunks );
	int64_t out_frames[2];
	for( int e = 0; e < 2; ++e )
		{
		const vec2d ear( 0, ( e == 0 ? 1 : -1 ) * head_width / 2.0f );
		for( int64_t k = 0; k < count; ++k ) dist[size_t( k )] = ( vec2d( ps[size_t( 64 * k )], ps[size_t( 64 * k + 1 )] ) - ear ).mag();
		out_frames[e] = flanhip_spatial_itd_out_frames( n, sr, dist.data(), count, stretches.data() + size_t( e * count ) );
		CHECK( out_frames[e] > 0 );
		}
	*frames = Frame( std::max( out_frames[0], out_frames[1] ) );
	std::vector<float> out( 2 * size_t( *frames ) );
	CHECK( flanhip_spatial_itd( shaped.data(), 2, n, sr, stretches.data(), count, out_frames, *frames, out.data(), nullptr ) == FLANHIP_OK );
	return out;
	}

static void device_checks()
	{
	const Frame n = 3001;
	const float sr = 48000.0f, step = 1.0f / sr;
	const size_t N = size_t( n );
	const std::vector<float> x = noise( N, 7 );
	const Audio a = Audio::create_from_buffer( std::vector<float>( x ), 1, sr );
	const float sqrt2 = std::sqrt( 2.0f );

	// a constant position: head_ild and falloff with one weight and one gain per ear, then a pure delay of Frame( n + delay ) frames (:139-153)
		{
		const Audio y = a.stereo_spatialize( vec2( 2, 1 ) );
		CHECK( !y.is_null() && y.is_device_resident() && !y.host_copy_is_current() );
		CHECK( y.get_num_channels() == 2 && y.get_sample_rate() == sr );
		std::vector<float> lp( N ), shaped( 2 * N );
		CHECK( flanhip_filter_1pole( x.data(), 1, n, sr, nullptr, 500.0f, FLANHIP_FILTER_BUTTERWORTH_LOW, 1, lp.data(), nullptr ) == FLANHIP_OK );
		CHECK( flanhip_spatial_ear( x.data(), lp.data(), 1, n, sr, nullptr, 2.0, 1.0, 0.18f, FLANHIP_SPATIAL_BOTH, shaped.data(), nullptr ) == FLANHIP_OK );
		Frame frames[2];
		float delay[2];
		for( int e = 0; e < 2; ++e )
			{
			const Meter dist = ( vec2d( 2, 1 ) - vec2d( 0, ( e == 0 ? 1 : -1 ) * 0.18f / 2.0f ) ).mag();
			delay[e] = ( dist / 343.0f ) * sr;
			frames[e] = Frame( n + delay[e] );
			}
		CHECK( frames[0] == n + 307 && frames[1] == n + 318 );                 // 2.197 m and 2.278 m at 343 m/s and 48 kHz
		CHECK( y.get_num_frames() == frames[1] );
		std::vector<float> want( 2 * size_t( frames[1] ), 0.0f );
		for( int e = 0; e < 2; ++e )
			for( Frame f = 0; f < n; ++f ) want[size_t( e ) * size_t( frames[1] ) + size_t( Frame( f + delay[e] ) )] = shaped[size_t( e ) * N + size_t( f )];
		CHECK( same_audio( y, want ) );
		// a constant samples nothing and is NOT the callable that returns it: that one goes through the resampler
		const Audio moving = a.stereo_spatialize( []( Second ){ return vec2( 2, 1 ); } );
		CHECK( !moving.is_null() && moving.get_num_channels() == 2 && !same_audio( moving, want ) );
		// the constant path has no shortest input
		const Audio tiny = Audio::create_from_buffer( noise( 20, 5 ), 1, sr );
		const Audio t = tiny.stereo_spatialize( vec2( 2, 1 ) );
		CHECK( !t.is_null() && t.get_num_frames() == 20 + 318 );
		}

	// a callable orbit, under the default speed limit and under one that bites, against the C ABI fed what the method samples
		{
		std::vector<double> ps( 2 * N );
		std::vector<float> fast( N, std::numeric_limits<float>::max() ), slow( N );
		for( Frame f = 0; f < n; ++f )
			{
			const vec2 v = orbit( f * step );
			ps[2 * size_t( f )] = v.x(); ps[2 * size_t( f ) + 1] = v.y();
			slow[size_t( f )] = 20.0f + 10.0f * sway( f * step );
			}
		Frame frames = 0;
		std::vector<float> want = spatialized( x, sr, ps, fast, 0.18f, &frames );
		const Audio y = a.stereo_spatialize( orbit );
		CHECK( !y.is_null() && y.is_device_resident() && y.get_num_channels() == 2 && y.get_num_frames() == frames );
		CHECK( same_audio( y, want ) );
		want = spatialized( x, sr, ps, slow, 0.3f, &frames );
		const Audio z = a.stereo_spatialize( orbit, 0.3f, []( Second t ){ return 20.0f + 10.0f * sway( t ); } );
		CHECK( z.get_num_frames() == frames && same_audio( z, want ) );
		CHECK( !same_audio( z, y.get_buffer() ) );
		}

	// 32 frames or fewer under a moving source: a null Audio and one line
		{
		std::ostringstream captured;
		std::streambuf * old = std::cout.rdbuf( captured.rdbuf() );
		const Audio tiny = Audio::create_from_buffer( noise( 32, 5 ), 1, sr );
		CHECK( tiny.stereo_spatialize( orbit ).is_null() );
		std::cout.rdbuf( old );
		CHECK( captured.str().find( "more than 32 frames" ) != std::string::npos );
		const Audio enough = Audio::create_from_buffer( noise( 33, 5 ), 1, sr );
		CHECK( !enough.stereo_spatialize( orbit ).is_null() );
		}

	// convert_to_stereo, convert_to_mono
	const std::vector<float> s = noise( 2 * N, 9 );
	const Audio st = Audio::create_from_buffer( std::vector<float>( s ), 2, sr );
		{
		std::vector<float> want( 2 * N );
		for( size_t f = 0; f < N; ++f ) want[f] = want[N + f] = x[f] / sqrt2;
		const Audio y = a.convert_to_stereo();
		CHECK( y.get_num_channels() == 2 && y.get_num_frames() == n && y.is_device_resident() && same_audio( y, want ) );
		CHECK( same_audio( st.convert_to_stereo(), s ) );
		const std::vector<float> t3 = noise( 3 * N, 11 );
		const Audio three = Audio::create_from_buffer( std::vector<float>( t3 ), 3, sr );
		std::vector<float> mono( N );
		for( size_t f = 0; f < N; ++f ) { float acc = 0; for( int c = 0; c < 3; ++c ) acc += t3[size_t( c ) * N + f]; mono[f] = acc / 3; }
		const Audio m = three.convert_to_mono();
		CHECK( m.get_num_channels() == 1 && m.get_num_frames() == n && same_audio( m, mono ) );
		CHECK( same_audio( a.convert_to_mono(), x ) );
		std::ostringstream captured;
		std::streambuf * old = std::cout.rdbuf( captured.rdbuf() );
		const Audio silent = three.convert_to_stereo();
		std::cout.rdbuf( old );
		CHECK( captured.str().find( "I don't know how to convert that number of channels to stereo." ) != std::string::npos );
		CHECK( same_audio( silent, std::vector<float>( 2 * N, 0.0f ) ) );
		}

	// pan on stereo and on mono, a constant and a callable, against the C ABI's host form; pan_in_place; widen
		{
		std::vector<float> want( 2 * N ), curve( N ), up( 2 * N );
		for( Frame f = 0; f < n; ++f ) curve[size_t( f )] = sway( f * step );
		CHECK( flanhip_audio_pan( s.data(), 2, n, nullptr, -0.25f, want.data(), nullptr ) == FLANHIP_OK );
		CHECK( same_audio( st.pan( -0.25f ), want ) );
		CHECK( same_audio( st.pan( []( Second ){ return -0.25f; } ), want ) );
		CHECK( flanhip_audio_pan( s.data(), 2, n, curve.data(), 0.0f, want.data(), nullptr ) == FLANHIP_OK );
		const Audio y = st.pan( sway );
		CHECK( y.is_device_resident() && same_audio( y, want ) );
		Audio mine = st.copy();
		CHECK( &mine.pan_in_place( sway ) == &mine && same_audio( mine, want ) );
		for( size_t f = 0; f < N; ++f ) up[f] = up[N + f] = x[f] / sqrt2;
		CHECK( flanhip_audio_pan( up.data(), 2, n, curve.data(), 0.0f, want.data(), nullptr ) == FLANHIP_OK );
		CHECK( same_audio( a.pan( sway ), want ) );
		Audio mono = a.copy();
		CHECK( mono.pan_in_place( sway ).get_num_channels() == 1 && same_audio( mono, x ) );       // :25: only stereo is panned in place
		// all the way to -1: channel 0 times sine2( 0 ) = 0, channel 1 times sine2( 1 ) = sqrt( 2 ) sin( pi / 4 ) = 1 within rounding
		const Audio end = st.pan( -1.0f );
		bool silent = true, close = true;
		for( size_t f = 0; f < N; ++f )
			{
			silent = silent && end.get_buffer()[f] == 0.0f;
			close = close && std::fabs( end.get_buffer()[N + f] - s[N + f] ) <= 1.2e-7f * std::fabs( s[N + f] );
			}
		CHECK( silent && close );
		const Audio w = st.widen( sway ), w2 = st.convert_to_mid_side().pan( sway ).convert_to_left_right();
		CHECK( !w.is_null() && same_audio( w, w2.get_buffer() ) && !same_audio( w, s ) );
		}

	// combine_channels of unequal lengths, zeros behind the shorter ones, and split_channels back
		{
		const std::vector<float> b = noise( 2 * 1001, 13 );
		const Audio shorter = Audio::create_from_buffer( std::vector<float>( b ), 2, sr );
		const Audio all = Audio::combine_channels( a, shorter, a );
		CHECK( all.get_num_channels() == 4 && all.get_num_frames() == n && all.is_device_resident() );
		std::vector<float> want( 4 * N, 0.0f );
		std::copy( x.begin(), x.end(), want.begin() );
		std::copy( b.begin(), b.begin() + 1001, want.begin() + N );
		std::copy( b.begin() + 1001, b.end(), want.begin() + 2 * N );
		std::copy( x.begin(), x.end(), want.begin() + 3 * N );
		CHECK( same_audio( all, want ) );
		CHECK( same_audio( Audio::combine_channels( std::vector<const Audio *>{ &a, &shorter, &a } ), want ) );
		const std::vector<Audio> parts = all.split_channels();
		CHECK( parts.size() == 4 );
		for( size_t c = 0; c < parts.size(); ++c )
			CHECK( parts[c].get_num_channels() == 1 && parts[c].get_num_frames() == n && parts[c].get_sample_rate() == sr
				&& same_audio( parts[c], std::vector<float>( want.begin() + c * N, want.begin() + ( c + 1 ) * N ) ) );
		CHECK( same_audio( Audio::combine_channels( parts ), want ) );
		// another sample rate: every input goes through Audio::resample to the highest one
		const Audio slow = Audio::create_from_buffer( noise( 500, 17 ), 1, 24000.0f );
		const Audio mixed = Audio::combine_channels( slow, a );
		const Audio slow_up = slow.resample( sr ), a_up = a.resample( sr );
		CHECK( mixed.get_sample_rate() == sr && mixed.get_num_channels() == 2 && mixed.get_num_frames() == std::max( slow_up.get_num_frames(), a_up.get_num_frames() ) );
		CHECK( same_audio( mixed, Audio::combine_channels( slow_up, a_up ).get_buffer() ) );
		}
	}

// spatial_test --bench SECONDS [STEPS WARMUP]: wall-clock medians for tools/bench_spatial.py, one JSON line per motion: the whole method
// (it synchronises before it returns), and on their own the sampling of the position and the speed limiter as the method runs them
static double median_ms( int steps, int warmup, const std::function<void()> & body )
	{
	std::vector<double> ms;
	for( int i = 0; i < warmup + steps; ++i )
		{
		const auto t0 = std::chrono::steady_clock::now();
		body();
		const auto t1 = std::chrono::steady_clock::now();
		if( i >= warmup ) ms.push_back( std::chrono::duration<double, std::milli>( t1 - t0 ).count() );
		}
	std::sort( ms.begin(), ms.end() );
	return ms.empty() ? 0.0 : ( ms[( ms.size() - 1 ) / 2] + ms[ms.size() / 2] ) / 2;
	}

static void bench( float seconds, int steps, int warmup )
	{
	const float sr = 48000.0f, step = 1.0f / sr;
	const Frame n = Frame( seconds * sr );
	const Audio a = Audio::create_from_buffer( noise( size_t( n ), 7 ), 1, sr );
	const float half = seconds / 2;
	const auto slow_orbit = []( Second t ){ return vec2( 2.0f * std::cos( pi * t ), 2.0f * std::sin( pi * t ) ); };        // radius 2 m, 0.5 Hz
	const auto fly_by = [half]( Second t ){ return vec2( 30.0f * ( t - half ), 2.0f ); };                                    // 30 m/s, 2 m off
	struct Motion { const char * name; std::function<vec2( Second )> fn; };
	const Motion motions[] = { { "slow orbit", slow_orbit }, { "fly-by", fly_by } };
	for( const Motion & m : motions )
		{
		Frame frames = 0;
		const double method = median_ms( steps, warmup, [&]{ const Audio y = a.stereo_spatialize( m.fn ); frames = y.get_num_frames(); CHECK( !y.is_null() ); } );
		std::vector<double> ps( 2 * size_t( n ) );
		const Function<Second, vec2> position( m.fn );
		const double sampling = median_ms( steps, warmup, [&]
			{
			detail::for_each_index( 0, n, position.get_execution_policy(), [&]( int x )
				{ const vec2 v = position( Second( x * step ) ); ps[2 * size_t( x )] = v.x(); ps[2 * size_t( x ) + 1] = v.y(); } );
			} );
		const std::vector<float> top( size_t( n ), std::numeric_limits<float>::max() );
		const double limiter = median_ms( steps, warmup, [&]{ std::vector<double> copy( ps ); limit( copy, top, sr ); } ),
			copying = median_ms( steps, warmup, [&]{ std::vector<double> copy( ps ); CHECK( copy.size() == ps.size() ); } );
		std::printf( "{\"shape\": \"%s\", \"in_frames\": %d, \"out_frames\": %d, \"method_ms_median\": %.3f, \"sampling_ms\": %.3f, \"limiter_ms\": %.3f}\n",
			m.name, n, frames, method, sampling, std::max( limiter - copying, 0.0 ) );
		}
	Frame frames = 0;
	const double method = median_ms( steps, warmup, [&]{ const Audio y = a.stereo_spatialize( vec2( 2, 1 ) ); frames = y.get_num_frames(); CHECK( !y.is_null() ); } );
	std::printf( "{\"shape\": \"constant position\", \"in_frames\": %d, \"out_frames\": %d, \"method_ms_median\": %.3f, \"sampling_ms\": 0, \"limiter_ms\": 0}\n", n, frames, method );
	}

int main( int argc, char ** argv )
	{
	const char * mode = argc > 1 ? argv[1] : "--no-device";
	if( !std::strcmp( mode, "--bench" ) )
		{
		if( flanhip_device_count() < 1 ) { std::printf( "FAILED: no device\n" ); return 1; }
		bench( argc > 2 ? float( std::atof( argv[2] ) ) : 60.0f, argc > 3 ? std::atoi( argv[3] ) : 10, argc > 4 ? std::atoi( argv[4] ) : 3 );
		return failures ? 1 : 0;
		}
	refusal_checks();
	if( !std::strcmp( mode, "--no-device" ) ) no_device_checks();
	if( !std::strcmp( mode, "--device" ) )
		{
		if( flanhip_device_count() < 1 ) { std::printf( "FAILED: no device\n" ); return 1; }
		device_checks();
		}
	std::printf( failures ? "%d FAILED\n" : "PASSED\n", failures );
	return failures ? 1 : 0;
	}
