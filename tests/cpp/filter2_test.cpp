// filter2_test.cpp -- Audio::filter_2pole_lowpass, _bandpass, _highpass, _notch, filter_2pole_lowshelf, _bandshelf, _highshelf and
// filter_1pole_lowshelf, _highshelf (include/flan/Audio.h) over libflan_host.so.
//   filter2_test --no-device  null in, null out for all nine; without a device the C ABI answers FLANHIP_ERR_NO_DEVICE and every method
//                             fails loudly with a null result
//   filter2_test --device     each method with constants and with callables against the C ABI's host form fed the scalars / the curves
//                             sampled where the reference samples them, bit for bit; the notch against the band-pass; the times the
//                             2-pole shelves sample at; order 0
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

static const auto sweep = []( Second t ){ return 300.0f + 20000.0f * t; };
static const auto damp = []( Second t ){ return 0.2f + 3.0f * t; };                 // 0.2 ... 0.76 over 9001 frames
static const auto swell = []( Second t ){ return -9.0f + 80.0f * t; };              // -9 ... +6 dB
// tells the two sampling times apart: where f * ( 1.0f / sr ) and f / sr differ in the last bit, so does this cutoff (1000 ... 4516 Hz)
static const auto bits_of_t = []( Second t ){ return 1000.0f + 4.0e5f * ( t - 0.09375f ) * ( t - 0.09375f ); };

static void null_checks()
	{
	std::ostringstream captured;                                               // "Null Audio created"
	std::streambuf * old = std::cout.rdbuf( captured.rdbuf() );
	CHECK( Audio().filter_2pole_lowpass( 1000.0f, 0.5f ).is_null() );
	CHECK( Audio().filter_2pole_bandpass( 1000.0f, 0.5f, 4 ).is_null() );
	CHECK( Audio().filter_2pole_highpass( sweep, damp, 3 ).is_null() );
	CHECK( Audio().filter_2pole_notch( 1000.0f, 0.5f, 0 ).is_null() );
	CHECK( Audio().filter_2pole_lowshelf( 1000.0f, 0.5f, 6.0f ).is_null() );
	CHECK( Audio().filter_2pole_bandshelf( sweep, damp, swell, 2 ).is_null() );
	CHECK( Audio().filter_2pole_highshelf( 1000.0f, 0.5f, 6.0f, 3 ).is_null() );
	CHECK( Audio().filter_1pole_lowshelf( 1000.0f, 6.0f ).is_null() );
	CHECK( Audio().filter_1pole_highshelf( sweep, swell, 2 ).is_null() );
	std::cout.rdbuf( old );
	CHECK( captured.str().find( "Null Audio created" ) != std::string::npos );
	}

static void no_device_checks()
	{
	void * bogus = reinterpret_cast<void*>( uintptr_t( 1 ) << 40 );           // never dereferenced
	const float * p = static_cast<const float*>( bogus );
	float * q = static_cast<float*>( bogus ) + 4096;
	CHECK( flanhip_filter2_dev( p, 2, 1000, 48000.0f, nullptr, 1000.0f, nullptr, 0.5f, nullptr, 6.0f, FLANHIP_FILTER2_LOW, 3, q, bogus, nullptr ) == FLANHIP_ERR_NO_DEVICE );
	const std::vector<float> x = noise( 2 * 1000, 1 );
	CHECK( flanhip_filter2( x.data(), 2, 1000, 48000.0f, nullptr, 1000.0f, nullptr, 0.5f, nullptr, 6.0f, FLANHIP_FILTER2_NOTCH, 0, q, nullptr ) == FLANHIP_ERR_NO_DEVICE );
	const Audio a = Audio::create_from_buffer( std::vector<float>( x ), 2, 48000.0f );
	std::ostringstream captured;
	std::streambuf * old = std::cout.rdbuf( captured.rdbuf() );
	CHECK( a.filter_2pole_lowpass( 1000.0f, 0.5f ).is_null() );
	CHECK( a.filter_2pole_bandpass( sweep, damp, 2 ).is_null() );
	CHECK( a.filter_2pole_highpass( 1000.0f, 0.5f, 0 ).is_null() );
	CHECK( a.filter_2pole_notch( 1000.0f, 0.5f, 2 ).is_null() );
	CHECK( a.filter_2pole_lowshelf( 1000.0f, 0.5f, 6.0f ).is_null() );
	CHECK( a.filter_2pole_bandshelf( 1000.0f, damp, 6.0f, 2 ).is_null() );
	CHECK( a.filter_2pole_highshelf( sweep, 0.5f, swell, 3 ).is_null() );
	CHECK( a.filter_1pole_lowshelf( 1000.0f, 6.0f ).is_null() );
	CHECK( a.filter_1pole_highshelf( 1000.0f, swell, 0 ).is_null() );
	std::cout.rdbuf( old );
	CHECK( !a.is_null() && same_bits( a.get_buffer().data(), x.data(), sizeof( float ) * x.size() ) );
	}

static void device_checks()
	{
	const Channel ch = 2;
	const Frame n = 9001;
	const float sr = 48000.0f;
	const std::vector<float> x = noise( size_t( ch ) * n, 7 );
	const Audio a = Audio::create_from_buffer( std::vector<float>( x ), ch, sr );
	std::vector<float> want( x.size() ), want2( x.size() );
	// the curves, sampled at f * ( 1.0f / sr ) (sample_function_over_domain) and at f / sr (frame_to_time)
	const size_t N = size_t( n );
	std::vector<float> c_mul( N ), d_mul( N ), g_mul( N ), c_div( N ), d_div( N ), t_mul( N ), t_div( N );
	const float step = 1.0f / sr;
	size_t times_differ = 0;
	for( Frame f = 0; f < n; ++f )
		{
		const float tm = f * step, td = float( f ) / sr;
		times_differ += tm != td;
		c_mul[size_t( f )] = sweep( tm ); d_mul[size_t( f )] = damp( tm ); g_mul[size_t( f )] = swell( tm ); t_mul[size_t( f )] = bits_of_t( tm );
		c_div[size_t( f )] = sweep( td ); d_div[size_t( f )] = damp( td ); t_div[size_t( f )] = bits_of_t( td );
		}
	CHECK( times_differ > 0 && !same_bits( t_mul.data(), t_div.data(), sizeof( float ) * N ) );
	auto abi = [&]( const float * cc, float c, const float * dc, float d, const float * gc, float g, int kind, int order, std::vector<float> & out )
		{
		return flanhip_filter2( x.data(), ch, n, sr, cc, c, dc, d, gc, g, kind, order, out.data(), nullptr ) == FLANHIP_OK;
		};

	// the Butterworth family: constants go as scalars, callables as curves sampled at f * ( 1.0f / sr ); the result stays in HBM until read
		{
		const Audio y = a.filter_2pole_lowpass( 1000.0f, 0.5f, 3 );
		CHECK( !y.is_null() && y.is_device_resident() && !y.host_copy_is_current() );
		CHECK( y.get_num_channels() == ch && y.get_num_frames() == n && y.get_sample_rate() == sr );
		CHECK( abi( nullptr, 1000.0f, nullptr, 0.5f, nullptr, 0.0f, FLANHIP_FILTER2_LOW, 3, want ) && same_audio( y, want ) );
		CHECK( !same_bits( want.data(), x.data(), sizeof( float ) * want.size() ) );       // it filtered something
		CHECK( abi( c_mul.data(), 0.0f, d_mul.data(), 0.0f, nullptr, 0.0f, FLANHIP_FILTER2_LOW, 4, want ) && same_audio( a.filter_2pole_lowpass( sweep, damp, 4 ), want ) );
		CHECK( abi( c_mul.data(), 0.0f, nullptr, 0.3f, nullptr, 0.0f, FLANHIP_FILTER2_LOW, 1, want ) && same_audio( a.filter_2pole_lowpass( sweep, 0.3f ), want ) );   // the default order
		CHECK( abi( nullptr, 800.0f, d_mul.data(), 0.0f, nullptr, 0.0f, FLANHIP_FILTER2_BAND, 2, want ) && same_audio( a.filter_2pole_bandpass( 800.0f, damp, 2 ), want ) );
		CHECK( abi( nullptr, 800.0f, nullptr, 0.25f, nullptr, 0.0f, FLANHIP_FILTER2_BAND, 1, want ) && same_audio( a.filter_2pole_bandpass( 800.0f, 0.25f ), want ) );
		CHECK( abi( c_mul.data(), 0.0f, d_mul.data(), 0.0f, nullptr, 0.0f, FLANHIP_FILTER2_HIGH, 5, want ) && same_audio( a.filter_2pole_highpass( sweep, damp, 5 ), want ) );
		CHECK( abi( nullptr, 500.0f, nullptr, 0.7f, nullptr, 0.0f, FLANHIP_FILTER2_HIGH, 2, want ) && same_audio( a.filter_2pole_highpass( 500.0f, 0.7f, 2 ), want ) );
		}

	// the notch is ( 0 + ( -band ) ) + x of the band-pass of the same arguments (:621-623); order 0 is silence
		{
		const Audio band = a.filter_2pole_bandpass( sweep, damp, 3 ), notch = a.filter_2pole_notch( sweep, damp, 3 );
		CHECK( !band.is_null() && !notch.is_null() && notch.is_device_resident() );
		if( !band.is_null() && !notch.is_null() )
			{
			for( size_t i = 0; i < x.size(); ++i ) want[i] = ( 0.0f + ( -band.get_buffer()[i] ) ) + x[i];
			CHECK( same_audio( notch, want ) );
			}
		CHECK( abi( c_mul.data(), 0.0f, d_mul.data(), 0.0f, nullptr, 0.0f, FLANHIP_FILTER2_NOTCH, 3, want2 ) && same_audio( notch, want2 ) );
		CHECK( abi( nullptr, 1000.0f, nullptr, 0.5f, nullptr, 0.0f, FLANHIP_FILTER2_NOTCH, 1, want ) && same_audio( a.filter_2pole_notch( 1000.0f, 0.5f ), want ) );
		const std::vector<float> zeros( x.size(), 0.0f );
		CHECK( same_audio( a.filter_2pole_notch( sweep, damp, 0 ), zeros ) );
		}

	// the 2-pole shelves sample cutoff and damping at f / sr, the gain at f * ( 1.0f / sr ) (:646-654)
		{
		CHECK( abi( nullptr, 1000.0f, nullptr, 0.5f, nullptr, 6.0f, FLANHIP_FILTER2_LOWSHELF, 1, want ) && same_audio( a.filter_2pole_lowshelf( 1000.0f, 0.5f, 6.0f ), want ) );
		CHECK( abi( c_div.data(), 0.0f, d_div.data(), 0.0f, g_mul.data(), 0.0f, FLANHIP_FILTER2_LOWSHELF, 3, want ) && same_audio( a.filter_2pole_lowshelf( sweep, damp, swell, 3 ), want ) );
		CHECK( abi( c_div.data(), 0.0f, nullptr, 0.4f, g_mul.data(), 0.0f, FLANHIP_FILTER2_BANDSHELF, 2, want ) && same_audio( a.filter_2pole_bandshelf( sweep, 0.4f, swell, 2 ), want ) );
		CHECK( abi( nullptr, 2000.0f, d_div.data(), 0.0f, nullptr, -6.0f, FLANHIP_FILTER2_BANDSHELF, 4, want ) && same_audio( a.filter_2pole_bandshelf( 2000.0f, damp, -6.0f, 4 ), want ) );
		CHECK( abi( c_div.data(), 0.0f, d_div.data(), 0.0f, g_mul.data(), 0.0f, FLANHIP_FILTER2_HIGHSHELF, 2, want ) && same_audio( a.filter_2pole_highshelf( sweep, damp, swell, 2 ), want ) );
		CHECK( abi( nullptr, 3000.0f, nullptr, 0.6f, nullptr, -12.0f, FLANHIP_FILTER2_HIGHSHELF, 3, want ) && same_audio( a.filter_2pole_highshelf( 3000.0f, 0.6f, -12.0f, 3 ), want ) );
		// a cutoff whose bits tell the two times apart: the method agrees with the curve sampled at f / sr and not with the other
		CHECK( abi( t_div.data(), 0.0f, nullptr, 0.5f, nullptr, 6.0f, FLANHIP_FILTER2_HIGHSHELF, 1, want ) );
		CHECK( abi( t_mul.data(), 0.0f, nullptr, 0.5f, nullptr, 6.0f, FLANHIP_FILTER2_HIGHSHELF, 1, want2 ) );
		CHECK( !same_bits( want.data(), want2.data(), sizeof( float ) * want.size() ) );
		CHECK( same_audio( a.filter_2pole_highshelf( bits_of_t, 0.5f, 6.0f ), want ) );
		// and the Butterworth family at f * ( 1.0f / sr )
		CHECK( abi( t_mul.data(), 0.0f, nullptr, 0.5f, nullptr, 0.0f, FLANHIP_FILTER2_LOW, 1, want ) && same_audio( a.filter_2pole_lowpass( bits_of_t, 0.5f ), want ) );
		}

	// the 1-pole shelves: cutoff and gain at f * ( 1.0f / sr )
		{
		CHECK( abi( nullptr, 1000.0f, nullptr, 0.0f, nullptr, 6.0f, FLANHIP_FILTER2_1POLE_LOWSHELF, 1, want ) && same_audio( a.filter_1pole_lowshelf( 1000.0f, 6.0f ), want ) );
		CHECK( abi( c_mul.data(), 0.0f, nullptr, 0.0f, g_mul.data(), 0.0f, FLANHIP_FILTER2_1POLE_LOWSHELF, 3, want ) && same_audio( a.filter_1pole_lowshelf( sweep, swell, 3 ), want ) );
		CHECK( abi( nullptr, 2000.0f, nullptr, 0.0f, g_mul.data(), 0.0f, FLANHIP_FILTER2_1POLE_HIGHSHELF, 2, want ) && same_audio( a.filter_1pole_highshelf( 2000.0f, swell, 2 ), want ) );
		CHECK( abi( c_mul.data(), 0.0f, nullptr, 0.0f, nullptr, -12.0f, FLANHIP_FILTER2_1POLE_HIGHSHELF, 1, want ) && same_audio( a.filter_1pole_highshelf( sweep, -12.0f ), want ) );
		}

	// order 0: copies; the 1-pole shelves times amp( gain / 2 )
		{
		CHECK( same_audio( a.filter_2pole_lowpass( 1000.0f, 0.5f, 0 ), x ) );
		CHECK( same_audio( a.filter_2pole_highshelf( sweep, damp, swell, 0 ), x ) );
		const float half = float( std::pow( 10.0, double( ( 6.0f / 2.0f ) / 20.0f ) ) );
		for( size_t i = 0; i < x.size(); ++i ) want[i] = x[i] * half;
		CHECK( same_audio( a.filter_1pole_lowshelf( 1000.0f, 6.0f, 0 ), want ) );
		CHECK( same_audio( a.filter_1pole_highshelf( sweep, 6.0f, 0 ), want ) );
		}
	}

int main( int argc, char ** argv )
	{
	const char * mode = argc > 1 ? argv[1] : "--no-device";
	null_checks();
	if( !std::strcmp( mode, "--no-device" ) ) no_device_checks();
	if( !std::strcmp( mode, "--device" ) )
		{
		if( flanhip_device_count() < 1 ) { std::printf( "FAILED: no device\n" ); return 1; }
		device_checks();
		}
	std::printf( failures ? "%d FAILED\n" : "PASSED\n", failures );
	return failures ? 1 : 0;
	}
