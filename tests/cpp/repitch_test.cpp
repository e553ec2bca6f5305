// repitch_test.cpp -- Audio::repitch (include/flan/Audio.h) over libflan_host.so.
//   repitch_test --no-device  null input and the Linear answer; without a device every other call fails loudly with a null result
//   repitch_test --device F   the same, and the cases of the raw fixture file F (tests/test_repitch_host_cpp.py writes it from
//                             tests/golden/ref_made/wdl_repitch.npz, with the factors BEFORE inversion) through Audio::repitch: the method's
//                             own sampling, inversion and clamp against the C ABI fed the fixture's inverted factors, bit for bit, and
//                             against the reference-made output; among them factors 0, negative and 1e-6 (both clamps), a step (a
//                             callable) and constants (the constant Function); then a ramp sampled at i * granularity, and the output
//                             length of a constant Function
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

static void null_and_linear_checks()
	{
	CHECK( Audio().repitch( 1.5f ).is_null() );
	const Audio a = Audio::create_from_buffer( noise( 2 * 1000, 1 ), 2, 48000.0f );
	std::ostringstream captured;
	std::streambuf * old = std::cout.rdbuf( captured.rdbuf() );
	const Audio lin = a.repitch( 1.5f, .001f, WDLResampleType::Linear );
	std::cout.rdbuf( old );
	CHECK( lin.is_null() );
	const std::string text = captured.str();
	size_t lines = 0;
	for( char c : text ) lines += c == '\n';
	CHECK( lines == 1 && text.find( "Linear" ) != std::string::npos && text.find( "not built" ) != std::string::npos );
	}

static void no_device_checks()
	{
	const Audio a = Audio::create_from_buffer( noise( 2 * 1000, 1 ), 2, 48000.0f );
	CHECK( a.repitch( 1.5f ).is_null() );
	CHECK( a.repitch( 0.7f, .001f, WDLResampleType::Uninterpolated ).is_null() );
	}

// fixture file: int32 cases; per case int32 ch, n, g, quality, count, out_frames; float sr; float x[ch n], factors[count], inv[count], out[ch out_frames]
static void fixture_checks( const char * path )
	{
	std::FILE * f = std::fopen( path, "rb" );
	if( !f ) { std::printf( "FAILED: cannot open %s\n", path ); ++failures; return; }
	int32_t cases = 0;
	CHECK( std::fread( &cases, 4, 1, f ) == 1 && cases > 0 );
	for( int32_t k = 0; k < cases; ++k )
		{
		int32_t h[6]; float sr;
		if( std::fread( h, 4, 6, f ) != 6 || std::fread( &sr, 4, 1, f ) != 1 ) { CHECK( false ); break; }
		const int32_t ch = h[0], n = h[1], g = h[2], quality = h[3], count = h[4], nout = h[5];
		std::vector<float> x( size_t( ch ) * n ), factors( count ), inv( count ), want( size_t( ch ) * nout );
		if( std::fread( x.data(), 4, x.size(), f ) != x.size() || std::fread( factors.data(), 4, factors.size(), f ) != factors.size()
			|| std::fread( inv.data(), 4, inv.size(), f ) != inv.size()
			|| std::fread( want.data(), 4, want.size(), f ) != want.size() ) { CHECK( false ); break; }
		// the factors as the caller gives them: a constant Function where they are all one value, else a callable that Audio::repitch
		// samples at i * granularity.  The inversion and the clamp are the method's: `inv` (what the reference's loop was fed) only goes
		// to the C ABI below.
		const Second gran = ( g + 0.5f ) / sr;                                   // Frame( gran * sr ) == g
		bool constant = true;
		for( int i = 1; i < count; ++i ) constant = constant && same_bits( &factors[size_t( i )], &factors[0], sizeof( float ) );
		const Function<Second, float> fn = constant ? Function<Second, float>( factors[0] ) : Function<Second, float>( [&]( Second t )
			{ const int i = int( std::floor( t / gran + 0.5f ) ); return factors[size_t( std::min( std::max( i, 0 ), count - 1 ) )]; } );
		const Audio a = Audio::create_from_buffer( std::vector<float>( x ), ch, sr );
		const Audio y = a.repitch( fn, gran, quality == 0 ? WDLResampleType::Sinc : WDLResampleType::Uninterpolated );
		CHECK( !y.is_null() && y.is_device_resident() );
		CHECK( y.get_num_channels() == ch && y.get_num_frames() == nout && y.get_sample_rate() == sr );
		if( y.is_null() || y.get_num_frames() != nout ) continue;
		std::vector<float> abi( want.size() );
		CHECK( flanhip_audio_repitch( x.data(), ch, n, sr, inv.data(), count, g, quality, abi.data(), nullptr ) == FLANHIP_OK );
		CHECK( same_bits( y.get_buffer().data(), abi.data(), sizeof( float ) * abi.size() ) );
		double num = 0.0, den = 0.0, peak = 0.0, worst = 0.0;
		for( size_t i = 0; i < want.size(); ++i )
			{
			const double d = double( y.get_buffer()[i] ) - want[i];
			num += d * d; den += double( want[i] ) * want[i];
			peak = std::max( peak, std::fabs( double( want[i] ) ) ); worst = std::max( worst, std::fabs( d ) );
			}
		const double rel_rms = den > 0 ? std::sqrt( num / den ) : std::sqrt( num ), rel_max = peak > 0 ? worst / peak : worst;
		std::printf( "case %d: ch %d n %d g %d q %d factor[0] %g -> %d frames  rel_rms %.3e rel_max %.3e\n", k, ch, n, g, quality, double( factors[0] ), nout, rel_rms, rel_max );
		CHECK( rel_rms <= 1.0e-6 && rel_max <= 1.0e-6 );                         // (the tight bounds are tests/test_gpu_repitch.py's)
		}
	std::fclose( f );
	}

// Function sampling: a callable is evaluated at i * granularity seconds, i = 0 .. ceil( n / float( g ) ) - 1 (AudioTemporal.cpp:245-249)
static void ramp_check()
	{
	const int ch = 2, n = 1000, g = 48;
	const Second gran = .001f;                                                   // 48 frames at 48 kHz
	const std::vector<float> x = noise( size_t( ch ) * n, 7 );
	std::vector<float> inv( 21 );                                                // ceil( 1000 / 48.f )
	for( int i = 0; i < 21; ++i ) inv[size_t( i )] = 1.0f / ( 0.5f + 50.0f * ( i * gran ) );   // 2 .. 1 / 1.5: inside the clamp
	const Audio a = Audio::create_from_buffer( std::vector<float>( x ), ch, 48000.0f );
	const Audio y = a.repitch( Function<Second, float>( []( Second t ){ return 0.5f + 50.0f * t; } ), gran );
	const int64_t nout = flanhip_audio_repitch_out_frames( inv.data(), 21, g );
	CHECK( !y.is_null() && y.get_num_channels() == ch && y.get_num_frames() == nout );
	if( y.is_null() || y.get_num_frames() != nout ) return;
	std::vector<float> abi( size_t( ch ) * size_t( nout ) );
	CHECK( flanhip_audio_repitch( x.data(), ch, n, 48000.0f, inv.data(), 21, g, FLANHIP_REPITCH_SINC, abi.data(), nullptr ) == FLANHIP_OK );
	CHECK( same_bits( y.get_buffer().data(), abi.data(), sizeof( float ) * abi.size() ) );
	}

// A stated deviation: the output length of a constant Function is the sequential fp32 sum of the inverted factor, as
// for the callable that returns the same value; the reference multiplies the constant by the count (FunctionSample.h:138-139).  One
// second at factor 1.5: 32001 frames here, ceil( ( 1 / 1.5f * 1000.f ) * 48.f ) = 32000 there.
static void constant_length_check()
	{
	const int n = 48000, g = 48, count = 1000;
	const Audio a = Audio::create_from_buffer( noise( size_t( n ), 9 ), 1, 48000.0f );
	const Audio y = a.repitch( 1.5f );
	const std::vector<float> inv( size_t( count ), 1.0f / 1.5f );
	const float product = ( inv[0] * float( count ) ) * float( g );
	CHECK( !y.is_null() && y.get_num_frames() == flanhip_audio_repitch_out_frames( inv.data(), count, g ) );
	CHECK( !y.is_null() && y.get_num_frames() == 32001 && int64_t( std::ceil( product ) ) == 32000 );
	}

int main( int argc, char ** argv )
	{
	const char * mode = argc > 1 ? argv[1] : "--no-device";
	null_and_linear_checks();
	if( !std::strcmp( mode, "--no-device" ) ) no_device_checks();
	if( !std::strcmp( mode, "--device" ) )
		{
		if( flanhip_device_count() < 1 ) { std::printf( "FAILED: no device\n" ); return 1; }
		if( argc < 3 ) { std::printf( "FAILED: no fixture file\n" ); return 1; }
		fixture_checks( argv[2] );
		ramp_check();
		constant_length_check();
		}
	std::printf( failures ? "%d FAILED\n" : "PASSED\n", failures );
	return failures ? 1 : 0;
	}
