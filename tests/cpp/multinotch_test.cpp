// multinotch_test.cpp -- Audio::filter_1pole_multinotch / filter_2pole_multinotch (include/flan/Audio.h) over libflan_host.so.
//   multinotch_test --no-device  null in, null out; the saturator, order 0 and an over-large order each give a message and a null Audio;
//                                without a device the C ABI answers FLANHIP_ERR_NO_DEVICE and the methods fail loudly with a null
//                                result, nothing sampled
//   multinotch_test --device     each method with constants and with callables against the C ABI's host form fed what the method samples,
//                                bit for bit
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

static const auto sweep = []( Second t ){ return 200.0f * std::pow( 40.0f, t * 5.0f ); };          // 200 Hz -> 8 kHz over 0.2 s
static const auto damp = []( Second t ){ return 0.3f + 4.0f * t; };
static const auto wobble = []( Second t ){ return 0.8f * std::sin( 90.0f * t ); };
static const auto mix = []( Second t ){ return 0.5f + 0.5f * std::cos( 40.0f * t ); };

// what needs no device: every refusal leaves a line on stderr and samples nothing
static void refusal_checks()
	{
	std::ostringstream captured, errors;                                       // "Null Audio created"
	std::streambuf * old = std::cout.rdbuf( captured.rdbuf() ), * old_err = std::cerr.rdbuf( errors.rdbuf() );
	CHECK( Audio().filter_1pole_multinotch( 4, 440.0f ).is_null() );
	CHECK( Audio().filter_2pole_multinotch( 4, sweep, damp, wobble, true, mix ).is_null() );
	CHECK( errors.str().empty() );                                             // null in, null out: nothing to report
	const std::vector<float> x = noise( 2 * 1000, 1 );
	const Audio a = Audio::create_from_buffer( std::vector<float>( x ), 2, 48000.0f );
	int sampled = 0;
	const Function<Second, Frequency> counted( [&]( Second ){ ++sampled; return 440.0f; }, ExecutionPolicy::Linear_Sequenced );
	auto refused = [&]( const Audio & y, const char * words )
		{
		CHECK( y.is_null() );
		CHECK( errors.str().find( words ) != std::string::npos );
		errors.str( "" );
		};
	refused( a.filter_1pole_multinotch( 4, counted, 0.5f, false, 0.5f, true ), "use_saturator" );
	refused( a.filter_2pole_multinotch( 4, counted, 0.7f, 0.5f, false, 0.5f, true ), "use_saturator" );
	refused( a.filter_1pole_multinotch( 0, counted ), "refused order 0" );
	refused( a.filter_2pole_multinotch( 0, counted, 0.7f ), "refused order 0" );
	refused( a.filter_1pole_multinotch( 17, counted ), "refused order 17" );
	refused( a.filter_2pole_multinotch( 9, counted, 0.7f ), "refused order 9" );
	refused( a.filter_2pole_multinotch( 65535, counted, 0.7f ), "refused order 65535" );
	std::cout.rdbuf( old ); std::cerr.rdbuf( old_err );
	CHECK( sampled == 0 );
	CHECK( captured.str().find( "Null Audio created" ) != std::string::npos );
	}

static void no_device_checks()
	{
	void * bogus = reinterpret_cast<void*>( uintptr_t( 1 ) << 40 );           // never dereferenced
	const float * p = static_cast<const float*>( bogus );
	float * q = static_cast<float*>( bogus ) + 4096;
	CHECK( flanhip_multinotch_dev( p, 2, 1000, 48000.0f, nullptr, 440.0f, nullptr, 0.7f, nullptr, 0.7f, nullptr, 0.5f, FLANHIP_MULTINOTCH_2POLE, 8, 0, q, bogus, nullptr ) == FLANHIP_ERR_NO_DEVICE );
	const std::vector<float> x = noise( 2 * 1000, 1 );
	std::vector<float> out( x.size() );
	CHECK( flanhip_multinotch( x.data(), 2, 1000, 48000.0f, nullptr, 440.0f, nullptr, 0.7f, nullptr, 0.7f, nullptr, 0.5f, FLANHIP_MULTINOTCH_1POLE, 16, 0, out.data(), nullptr ) == FLANHIP_ERR_NO_DEVICE );
	const Audio a = Audio::create_from_buffer( std::vector<float>( x ), 2, 48000.0f );
	std::ostringstream captured;
	std::streambuf * old = std::cout.rdbuf( captured.rdbuf() );
	int sampled = 0;
	const Function<Second, Frequency> counted( [&]( Second ){ ++sampled; return 440.0f; }, ExecutionPolicy::Linear_Sequenced );
	CHECK( a.filter_1pole_multinotch( 4, 440.0f, 0.7f ).is_null() );
	CHECK( a.filter_1pole_multinotch( 4, counted, wobble, false, mix ).is_null() );
	CHECK( a.filter_2pole_multinotch( 4, counted, damp, wobble, true, mix ).is_null() );
	std::cout.rdbuf( old );
	CHECK( sampled == 0 );                                                     // without a device nothing is sampled
	CHECK( !a.is_null() && same_bits( a.get_buffer().data(), x.data(), sizeof( float ) * x.size() ) );
	}

static void device_checks()
	{
	const Channel ch = 2;
	const Frame n = 9001;
	const float sr = 48000.0f;
	const size_t N = size_t( n );
	const std::vector<float> x = noise( size_t( ch ) * n, 7 );
	const Audio a = Audio::create_from_buffer( std::vector<float>( x ), ch, sr );
	std::vector<float> want( x.size() );
	const float step = 1.0f / sr;
	const int P1 = FLANHIP_MULTINOTCH_1POLE, P2 = FLANHIP_MULTINOTCH_2POLE;

	// constants go as scalars; the defaults are feedback 0, not inverted, wet_dry .5; the result stays in HBM until read
		{
		const Audio y = a.filter_1pole_multinotch( 6, 440.0f, 0.7f, true, 0.25f );
		CHECK( !y.is_null() && y.is_device_resident() && !y.host_copy_is_current() );
		CHECK( y.get_num_channels() == ch && y.get_num_frames() == n && y.get_sample_rate() == sr );
		CHECK( flanhip_multinotch( x.data(), ch, n, sr, nullptr, 440.0f, nullptr, 0.0f, nullptr, 0.7f, nullptr, 0.25f, P1, 6, 1, want.data(), nullptr ) == FLANHIP_OK && same_audio( y, want ) );
		CHECK( !same_bits( want.data(), x.data(), sizeof( float ) * want.size() ) );
		CHECK( flanhip_multinotch( x.data(), ch, n, sr, nullptr, 440.0f, nullptr, 0.0f, nullptr, 0.0f, nullptr, 0.5f, P1, 16, 0, want.data(), nullptr ) == FLANHIP_OK );
		CHECK( same_audio( a.filter_1pole_multinotch( 16, 440.0f ), want ) );
		// a constant samples nothing and equals the callable that returns it
		CHECK( same_audio( a.filter_1pole_multinotch( 16, []( Second ){ return 440.0f; }, []( Second ){ return 0.0f; }, false, []( Second ){ return 0.5f; } ), want ) );
		CHECK( flanhip_multinotch( x.data(), ch, n, sr, nullptr, 440.0f, nullptr, 0.6f, nullptr, -0.7f, nullptr, 0.25f, P2, 3, 1, want.data(), nullptr ) == FLANHIP_OK );
		CHECK( same_audio( a.filter_2pole_multinotch( 3, 440.0f, 0.6f, -0.7f, true, 0.25f ), want ) );
		CHECK( flanhip_multinotch( x.data(), ch, n, sr, nullptr, 440.0f, nullptr, 0.6f, nullptr, 0.0f, nullptr, 0.5f, P2, 8, 0, want.data(), nullptr ) == FLANHIP_OK );
		CHECK( same_audio( a.filter_2pole_multinotch( 8, 440.0f, 0.6f ), want ) );
		CHECK( same_audio( a.filter_2pole_multinotch( 8, []( Second ){ return 440.0f; }, []( Second ){ return 0.6f; } ), want ) );
		}

	// callables are sampled once per frame at f * ( 1.0f / sr ), each on its own
		{
		std::vector<float> c( N ), R( N ), k( N ), m( N );
		for( Frame f = 0; f < n; ++f )
			{ c[size_t( f )] = sweep( f * step ); R[size_t( f )] = damp( f * step ); k[size_t( f )] = wobble( f * step ); m[size_t( f )] = mix( f * step ); }
		CHECK( flanhip_multinotch( x.data(), ch, n, sr, c.data(), 0.0f, nullptr, 0.0f, k.data(), 0.0f, m.data(), 0.0f, P1, 5, 0, want.data(), nullptr ) == FLANHIP_OK );
		CHECK( same_audio( a.filter_1pole_multinotch( 5, sweep, wobble, false, mix ), want ) );
		CHECK( flanhip_multinotch( x.data(), ch, n, sr, c.data(), 0.0f, nullptr, 0.0f, nullptr, 0.9f, m.data(), 0.0f, P1, 2, 1, want.data(), nullptr ) == FLANHIP_OK );
		CHECK( same_audio( a.filter_1pole_multinotch( 2, sweep, 0.9f, true, mix ), want ) );
		CHECK( flanhip_multinotch( x.data(), ch, n, sr, c.data(), 0.0f, R.data(), 0.0f, k.data(), 0.0f, m.data(), 0.0f, P2, 4, 1, want.data(), nullptr ) == FLANHIP_OK );
		CHECK( same_audio( a.filter_2pole_multinotch( 4, sweep, damp, wobble, true, mix ), want ) );
		CHECK( flanhip_multinotch( x.data(), ch, n, sr, nullptr, 2000.0f, R.data(), 0.0f, nullptr, 0.5f, nullptr, 1.0f, P2, 7, 0, want.data(), nullptr ) == FLANHIP_OK );
		CHECK( same_audio( a.filter_2pole_multinotch( 7, 2000.0f, damp, 0.5f, false, 1.0f ), want ) );
		}
	}

int main( int argc, char ** argv )
	{
	const char * mode = argc > 1 ? argv[1] : "--no-device";
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
