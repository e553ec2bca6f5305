// filter_test.cpp -- Audio::filter_1pole_lowpass, _highpass, _split, _repeat_low and _repeat_high (include/flan/Audio.h) over libflan_host.so.
//   filter_test --no-device  null in, null out for all five; without a device the C ABI answers FLANHIP_ERR_NO_DEVICE and every method
//                            fails loudly with a null result
//   filter_test --device     each method with a constant and with a callable cutoff against the C ABI's host form fed the scalar / the
//                            curve sampled at f * frame_to_time( 1 ), bit for bit; split at orders 1 and 4 against the compositions it
//                            stands for; order 0 and no repeats; and a chain convert_to_PV -> convert_to_audio -> filter_1pole_highpass
//                            -> set_volume that stays in HBM
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

static void null_checks()
	{
	std::ostringstream captured;                                               // "Null Audio created"
	std::streambuf * old = std::cout.rdbuf( captured.rdbuf() );
	CHECK( Audio().filter_1pole_lowpass( 1000.0f ).is_null() );
	CHECK( Audio().filter_1pole_highpass( 1000.0f, 4 ).is_null() );
	CHECK( Audio().filter_1pole_repeat_low( 1000.0f, 3 ).is_null() );
	CHECK( Audio().filter_1pole_repeat_high( sweep, 0 ).is_null() );
	const std::vector<Audio> split = Audio().filter_1pole_split( 1000.0f, 4 );
	CHECK( split.size() == 2 && split[0].is_null() && split[1].is_null() );
	std::cout.rdbuf( old );
	CHECK( captured.str().find( "Null Audio created" ) != std::string::npos );
	}

static void no_device_checks()
	{
	void * bogus = reinterpret_cast<void*>( uintptr_t( 1 ) << 40 );           // never dereferenced
	const float * p = static_cast<const float*>( bogus );
	float * q = static_cast<float*>( bogus );
	CHECK( flanhip_filter_1pole_dev( p, 2, 1000, 48000.0f, nullptr, 1000.0f, FLANHIP_FILTER_BUTTERWORTH_LOW, 3, q, bogus, nullptr ) == FLANHIP_ERR_NO_DEVICE );
	const std::vector<float> x = noise( 2 * 1000, 1 );
	CHECK( flanhip_filter_1pole( x.data(), 2, 1000, 48000.0f, nullptr, 1000.0f, FLANHIP_FILTER_REPEAT_HIGH, 0, q, nullptr ) == FLANHIP_ERR_NO_DEVICE );
	const Audio a = Audio::create_from_buffer( std::vector<float>( x ), 2, 48000.0f );
	std::ostringstream captured;
	std::streambuf * old = std::cout.rdbuf( captured.rdbuf() );
	CHECK( a.filter_1pole_lowpass( 1000.0f ).is_null() );
	CHECK( a.filter_1pole_highpass( sweep, 2 ).is_null() );
	CHECK( a.filter_1pole_repeat_low( 1000.0f, 2 ).is_null() );
	CHECK( a.filter_1pole_repeat_high( 1000.0f, 0 ).is_null() );
	const std::vector<Audio> split = a.filter_1pole_split( 1000.0f, 2 );
	CHECK( split.size() == 2 && split[0].is_null() && split[1].is_null() );
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
	std::vector<float> want( x.size() ), want2( x.size() ), curve( static_cast<size_t>( n ) );
	const float step = a.frame_to_time( 1 );
	for( Frame f = 0; f < n; ++f ) curve[size_t( f )] = sweep( f * step );
	auto abi = [&]( const std::vector<float> & in, const float * cutoff_curve, float cutoff, int kind, int order, std::vector<float> & out )
		{
		return flanhip_filter_1pole( in.data(), ch, n, sr, cutoff_curve, cutoff, kind, order, out.data(), nullptr ) == FLANHIP_OK;
		};

	// each method: a constant goes as the scalar, a callable as the curve sampled once per frame; the result stays in HBM until read
		{
		const Audio y = a.filter_1pole_lowpass( 1000.0f, 3 );
		CHECK( !y.is_null() && y.is_device_resident() && !y.host_copy_is_current() );
		CHECK( y.get_num_channels() == ch && y.get_num_frames() == n && y.get_sample_rate() == sr );
		CHECK( abi( x, nullptr, 1000.0f, FLANHIP_FILTER_BUTTERWORTH_LOW, 3, want ) && same_audio( y, want ) );
		CHECK( !same_bits( want.data(), x.data(), sizeof( float ) * want.size() ) );       // it filtered something
		CHECK( abi( x, curve.data(), 0.0f, FLANHIP_FILTER_BUTTERWORTH_LOW, 4, want ) && same_audio( a.filter_1pole_lowpass( sweep, 4 ), want ) );
		CHECK( abi( x, nullptr, 1000.0f, FLANHIP_FILTER_BUTTERWORTH_LOW, 1, want ) && same_audio( a.filter_1pole_lowpass( 1000.0f ), want ) );   // the default order
		CHECK( abi( x, nullptr, 500.0f, FLANHIP_FILTER_BUTTERWORTH_HIGH, 2, want ) && same_audio( a.filter_1pole_highpass( 500.0f, 2 ), want ) );
		CHECK( abi( x, curve.data(), 0.0f, FLANHIP_FILTER_BUTTERWORTH_HIGH, 5, want ) && same_audio( a.filter_1pole_highpass( sweep, 5 ), want ) );
		CHECK( abi( x, curve.data(), 0.0f, FLANHIP_FILTER_BUTTERWORTH_HIGH, 1, want ) && same_audio( a.filter_1pole_highpass( sweep ), want ) );
		CHECK( abi( x, nullptr, 2000.0f, FLANHIP_FILTER_REPEAT_LOW, 5, want ) && same_audio( a.filter_1pole_repeat_low( 2000.0f, 5 ), want ) );
		CHECK( abi( x, curve.data(), 0.0f, FLANHIP_FILTER_REPEAT_LOW, 2, want ) && same_audio( a.filter_1pole_repeat_low( sweep, 2 ), want ) );
		CHECK( abi( x, nullptr, 2000.0f, FLANHIP_FILTER_REPEAT_HIGH, 3, want ) && same_audio( a.filter_1pole_repeat_high( 2000.0f, 3 ), want ) );
		CHECK( abi( x, curve.data(), 0.0f, FLANHIP_FILTER_REPEAT_HIGH, 1, want ) && same_audio( a.filter_1pole_repeat_high( sweep, 1 ), want ) );
		}

	// split: order <= 1 is { low( 1 ), high( 1 ) }; above, each filter twice over (:406-422)
		{
		const std::vector<Audio> one = a.filter_1pole_split( sweep );
		CHECK( one.size() == 2 && one[0].is_device_resident() && one[1].is_device_resident() );
		CHECK( abi( x, curve.data(), 0.0f, FLANHIP_FILTER_BUTTERWORTH_LOW, 1, want ) && one.size() == 2 && same_audio( one[0], want ) );
		CHECK( abi( x, curve.data(), 0.0f, FLANHIP_FILTER_BUTTERWORTH_HIGH, 1, want ) && one.size() == 2 && same_audio( one[1], want ) );
		const std::vector<Audio> zero = a.filter_1pole_split( sweep, 0 );                  // order 0 is order 1 here
		CHECK( zero.size() == 2 && same_audio( zero[1], want ) );
		const std::vector<Audio> four = a.filter_1pole_split( 1500.0f, 4 );
		CHECK( abi( x, nullptr, 1500.0f, FLANHIP_FILTER_BUTTERWORTH_LOW, 4, want ) && abi( want, nullptr, 1500.0f, FLANHIP_FILTER_BUTTERWORTH_LOW, 4, want2 ) );
		CHECK( four.size() == 2 && same_audio( four[0], want2 ) );
		CHECK( abi( x, nullptr, 1500.0f, FLANHIP_FILTER_BUTTERWORTH_HIGH, 4, want ) && abi( want, nullptr, 1500.0f, FLANHIP_FILTER_BUTTERWORTH_HIGH, 4, want2 ) );
		CHECK( four.size() == 2 && same_audio( four[1], want2 ) );
		CHECK( four.size() == 2 && same_audio( a.filter_1pole_highpass( 1500.0f, 4 ).filter_1pole_highpass( 1500.0f, 4 ), four[1].get_buffer() ) );
		}

	// order 0 copies; no repeats are silence
		{
		CHECK( same_audio( a.filter_1pole_lowpass( 1000.0f, 0 ), x ) );
		CHECK( same_audio( a.filter_1pole_highpass( sweep, 0 ), x ) );
		const std::vector<float> zeros( x.size(), 0.0f );
		CHECK( same_audio( a.filter_1pole_repeat_low( 1000.0f, 0 ), zeros ) );
		CHECK( same_audio( a.filter_1pole_repeat_high( sweep, 0 ), zeros ) );
		}

	// a chain that never leaves the device: rumble taken out after a phase-vocoder round trip
		{
		const PV pv = a.convert_to_PV( 2048, 512, 2048 );
		const Audio back = pv.convert_to_audio();
		const Audio filtered = back.filter_1pole_highpass( 30.0f, 2 );
		const Audio level = filtered.set_volume( 0.9f );
		CHECK( !pv.is_null() && pv.is_device_resident() && !pv.host_copy_is_current() );
		CHECK( !back.is_null() && back.is_device_resident() && !back.host_copy_is_current() );
		CHECK( !filtered.is_null() && filtered.is_device_resident() && !filtered.host_copy_is_current() );
		CHECK( !level.is_null() && level.is_device_resident() && !level.host_copy_is_current() );
		const Audio chained = a.convert_to_PV( 2048, 512, 2048 ).convert_to_audio().filter_1pole_highpass( 30.0f, 2 ).set_volume( 0.9f );
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
