// compress_test.cpp -- Audio::compress, modify_volume and set_volume (include/flan/Audio.h) over libflan_host.so.
//   compress_test --no-device  null in, null out; the short and the null sidechain; without a device the C ABI answers FLANHIP_ERR_NO_DEVICE
//                              and every method fails loudly with a null result (the in-place forms leave the object as it is)
//   compress_test --device     the same refusals, and: compress with constant and with callable Functions against the C ABI fed the
//                              scalars / the curves sampled at f * frame_to_time( 1 ), bit for bit; a mono and a longer sidechain;
//                              modify_volume and set_volume against the host arithmetic of the reference, bit for bit; the in-place
//                              forms; and a chain convert_to_PV -> convert_to_audio -> compress -> set_volume that stays in HBM
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <vector>

#include "flan/flan.h"
#include "flanhip.h"

using namespace flan;

static int failures = 0;
#define CHECK( cond ) do { if( !( cond ) ) { std::printf( "FAILED: %s (line %d)\n", #cond, __LINE__ ); ++failures; } } while( 0 )

static bool same_bits( const void * a, const void * b, size_t bytes ) { return std::memcmp( a, b, bytes ) == 0; }

static std::vector<float> noise( size_t n, uint32_t seed )
	{
	std::vector<float> v( n );
	for( size_t i = 0; i < n; ++i ) { seed = seed * 1664525u + 1013904223u; v[i] = float( int32_t( seed >> 8 ) - ( 1 << 23 ) ) / float( 1 << 24 ); }
	return v;
	}

// bursts: loud and quiet stretches of 300 frames, so that the detector attacks and releases
static std::vector<float> bursts( Channel ch, Frame n, uint32_t seed )
	{
	std::vector<float> v = noise( size_t( ch ) * n, seed );
	for( Channel c = 0; c < ch; ++c )
		for( Frame f = 0; f < n; ++f ) v[size_t( c ) * n + f] *= ( f / 300 ) % 2 == 0 ? 1.0f : 0.02f;
	return v;
	}

static void null_and_refusal_checks()
	{
	std::ostringstream captured;                                               // "Null Audio created" and the refusal's line
	std::streambuf * old = std::cout.rdbuf( captured.rdbuf() );
	CHECK( Audio().compress( -20.0f ).is_null() );
	CHECK( Audio().modify_volume( 0.5f ).is_null() );
	CHECK( Audio().set_volume( 0.5f ).is_null() );
	Audio null_audio;
	CHECK( null_audio.modify_volume_in_place( 0.5f ).is_null() && null_audio.set_volume_in_place( 0.5f ).is_null() );
	const Audio a = Audio::create_from_buffer( noise( 2 * 1000, 1 ), 2, 48000.0f );
	const Audio shorter = Audio::create_from_buffer( noise( 999, 2 ), 1, 48000.0f );
	const Audio none;
	CHECK( a.compress( -20.0f, 3.0f, 0.005f, 0.1f, 0.0f, &shorter ).is_null() );
	CHECK( a.compress( -20.0f, 3.0f, 0.005f, 0.1f, 0.0f, &none ).is_null() );
	std::cout.rdbuf( old );
	CHECK( captured.str().find( "fewer frames" ) != std::string::npos );
	}

static void no_device_checks()
	{
	void * bogus = reinterpret_cast<void*>( uintptr_t( 1 ) << 40 );           // never dereferenced
	const float * p = static_cast<const float*>( bogus );
	float * q = static_cast<float*>( bogus );
	CHECK( flanhip_compress_dev( p, 2, 1000, 48000.0f, p, 2, 1000, nullptr, -20.0f, nullptr, 3.0f, nullptr, 0.005f, nullptr, 0.1f, nullptr, 0.0f,
		q, nullptr, bogus, nullptr ) == FLANHIP_ERR_NO_DEVICE );
	CHECK( flanhip_audio_gain_dev( p, 2, 1000, nullptr, 0.5f, q, nullptr ) == FLANHIP_ERR_NO_DEVICE );
	CHECK( flanhip_audio_set_volume_dev( p, 2, 1000, 48000.0f, nullptr, 0.5f, q, bogus, nullptr ) == FLANHIP_ERR_NO_DEVICE );
	const std::vector<float> x = noise( 2 * 1000, 1 );
	Audio a = Audio::create_from_buffer( std::vector<float>( x ), 2, 48000.0f );
	CHECK( a.compress( -20.0f ).is_null() );
	CHECK( a.modify_volume( 0.5f ).is_null() );
	CHECK( a.set_volume( 0.5f ).is_null() );
	a.modify_volume_in_place( 0.5f ).set_volume_in_place( 0.5f );
	CHECK( !a.is_null() && same_bits( a.get_buffer().data(), x.data(), sizeof( float ) * x.size() ) );
	}

static void device_checks()
	{
	const Channel ch = 2;
	const Frame n = 9001;
	const float sr = 48000.0f;
	const std::vector<float> x = bursts( ch, n, 7 );
	const Audio a = Audio::create_from_buffer( std::vector<float>( x ), ch, sr );
	std::vector<float> want( x.size() );

	// constant Functions: the C ABI's host form with scalars, bit for bit; the result stays in HBM until read
		{
		const Audio y = a.compress( -20.0f, 3.0f, 0.005f, 0.1f, 6.0f );
		CHECK( !y.is_null() && y.is_device_resident() && !y.host_copy_is_current() );
		CHECK( y.get_num_channels() == ch && y.get_num_frames() == n && y.get_sample_rate() == sr );
		CHECK( flanhip_compress( x.data(), ch, n, sr, x.data(), ch, n, nullptr, -20.0f, nullptr, 3.0f, nullptr, 0.005f, nullptr, 0.1f, nullptr, 6.0f,
			want.data(), nullptr, nullptr ) == FLANHIP_OK );
		CHECK( !y.is_null() && same_bits( y.get_buffer().data(), want.data(), sizeof( float ) * want.size() ) );
		CHECK( !same_bits( want.data(), x.data(), sizeof( float ) * want.size() ) );      // it compressed something
		const Audio d = a.compress( -20.0f );                                              // the defaults: 3, 5 ms, 100 ms, no knee
		CHECK( flanhip_compress( x.data(), ch, n, sr, x.data(), ch, n, nullptr, -20.0f, nullptr, 3.0f, nullptr, 5.0f / 1000.0f, nullptr, 100.0f / 1000.0f,
			nullptr, 0.0f, want.data(), nullptr, nullptr ) == FLANHIP_OK );
		CHECK( !d.is_null() && same_bits( d.get_buffer().data(), want.data(), sizeof( float ) * want.size() ) );
		}

	// callables: sampled once per frame at f * frame_to_time( 1 ) (:220-224); a mono sidechain, and a longer one read up to n
		{
		const float step = a.frame_to_time( 1 );
		std::vector<float> thr( n ), att( n );
		for( Frame f = 0; f < n; ++f ) { thr[size_t( f )] = -30.0f + 100.0f * ( f * step ); att[size_t( f )] = ( f * step ) < 0.1f ? 0.0005f : 0.02f; }
		const std::vector<float> sv = bursts( 1, n + 500, 8 );
		const Audio side = Audio::create_from_buffer( std::vector<float>( sv ), 1, 44100.0f );   // its rate is not looked at
		const Audio y = a.compress( []( Second t ){ return -30.0f + 100.0f * t; }, 4.0f, []( Second t ){ return t < 0.1f ? 0.0005f : 0.02f; }, 0.05f, 3.0f, &side );
		CHECK( !y.is_null() && y.is_device_resident() );
		CHECK( flanhip_compress( x.data(), ch, n, sr, sv.data(), 1, n + 500, thr.data(), 0.0f, nullptr, 4.0f, att.data(), 0.0f, nullptr, 0.05f, nullptr, 3.0f,
			want.data(), nullptr, nullptr ) == FLANHIP_OK );
		CHECK( !y.is_null() && same_bits( y.get_buffer().data(), want.data(), sizeof( float ) * want.size() ) );
		}

	// modify_volume: one fp32 product per sample, a constant and a callable sampled at f * ( 1.0f / sr ); the in-place form
		{
		const Audio y = a.modify_volume( 0.3f );
		const Audio z = a.modify_volume( []( Second t ){ return 1.0f - 2.0f * t; } );
		CHECK( !y.is_null() && y.is_device_resident() && !z.is_null() && z.is_device_resident() );
		size_t bad = 0;
		for( Channel c = 0; c < ch && !y.is_null() && !z.is_null(); ++c )
			for( Frame f = 0; f < n; ++f )
				{
				const size_t i = size_t( c ) * n + f;
				const float wy = x[i] * 0.3f, wz = x[i] * ( 1.0f - 2.0f * ( f * ( 1.0f / sr ) ) );
				bad += !same_bits( &wy, &y.get_buffer()[i], 4 ) + !same_bits( &wz, &z.get_buffer()[i], 4 );
				}
		CHECK( bad == 0 );
		Audio w = a.copy();
		Audio & back = w.modify_volume_in_place( 0.3f );
		CHECK( &back == &w && !y.is_null() && same_bits( w.get_buffer().data(), y.get_buffer().data(), sizeof( float ) * x.size() ) );
		}

	// set_volume: level / get_max_sample_magnitude(), one division and one product (:63-66); the last frame is not looked at
		{
		std::vector<float> v = x;
		v[size_t( n ) - 1] = 3.0f;                                                         // the peak, where the maximum does not look
		const Audio b = Audio::create_from_buffer( std::vector<float>( v ), ch, sr );
		const float m = b.get_max_sample_magnitude();
		CHECK( m > 0.0f && m < 1.0f );
		const Audio y = b.set_volume( 0.9f );
		const Audio z = b.set_volume( []( Second t ){ return 0.5f + t; } );
		CHECK( !y.is_null() && y.is_device_resident() && !y.host_copy_is_current() && !z.is_null() );
		size_t bad = 0;
		for( Channel c = 0; c < ch && !y.is_null() && !z.is_null(); ++c )
			for( Frame f = 0; f < n; ++f )
				{
				const size_t i = size_t( c ) * n + f;
				const float wy = v[i] * ( 0.9f / m ), wz = v[i] * ( ( 0.5f + f * ( 1.0f / sr ) ) / m );
				bad += !same_bits( &wy, &y.get_buffer()[i], 4 ) + !same_bits( &wz, &z.get_buffer()[i], 4 );
				}
		CHECK( bad == 0 );
		Audio w = b.copy();
		w.set_volume_in_place( 0.9f );
		CHECK( !y.is_null() && same_bits( w.get_buffer().data(), y.get_buffer().data(), sizeof( float ) * v.size() ) );
		const Audio silent = Audio::create_empty_with_frames( 1000, 2, sr ).set_volume( 0.9f );   // a maximum of 0: unchanged, not NaN
		size_t nonzero = 0;
		for( float s : silent.get_buffer() ) nonzero += !( s == 0.0f );
		CHECK( !silent.is_null() && nonzero == 0 );
		}

	// a chain that never leaves the device: the mastering step after a phase-vocoder round trip
		{
		const PV pv = a.convert_to_PV( 2048, 512, 2048 );
		const Audio back = pv.convert_to_audio();
		const Audio squeezed = back.compress( -20.0f, 4.0f );
		const Audio level = squeezed.set_volume( 0.9f );
		CHECK( !pv.is_null() && pv.is_device_resident() && !pv.host_copy_is_current() );
		CHECK( !back.is_null() && back.is_device_resident() && !back.host_copy_is_current() );
		CHECK( !squeezed.is_null() && squeezed.is_device_resident() && !squeezed.host_copy_is_current() );
		CHECK( !level.is_null() && level.is_device_resident() && !level.host_copy_is_current() );
		const Audio chained = a.convert_to_PV( 2048, 512, 2048 ).convert_to_audio().compress( -20.0f, 4.0f ).set_volume( 0.9f );
		CHECK( !chained.is_null() && chained.is_device_resident() && !chained.host_copy_is_current() );
		if( !chained.is_null() && !level.is_null() )
			{
			CHECK( same_bits( chained.get_buffer().data(), level.get_buffer().data(), sizeof( float ) * level.get_buffer().size() ) );
			const float m = chained.get_max_sample_magnitude();
			CHECK( std::fabs( m - 0.9f ) <= 1e-6f );
			}
		}
	}

int main( int argc, char ** argv )
	{
	const char * mode = argc > 1 ? argv[1] : "--no-device";
	null_and_refusal_checks();
	if( !std::strcmp( mode, "--no-device" ) ) no_device_checks();
	if( !std::strcmp( mode, "--device" ) )
		{
		if( flanhip_device_count() < 1 ) { std::printf( "FAILED: no device\n" ); return 1; }
		device_checks();
		}
	std::printf( failures ? "%d FAILED\n" : "PASSED\n", failures );
	return failures ? 1 : 0;
	}
