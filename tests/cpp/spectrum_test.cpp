// spectrum_test.cpp -- Audio::synthesize_spectrum (include/flan/Audio.h) over libflan_host.so.
//   spectrum_test --no-device      invalid arguments give null Audios; a size the library does not serve gives a null Audio and a line on stderr;
//                                  without a device a valid call gives a null Audio, loudly
//   spectrum_test --device         the method with explicit phases equals flanhip_audio_synthesize_spectrum on the same arrays, bit for bit, at a
//                                  one-workgroup and at a two-pass size; the peak is 1; without phases two calls differ and each peaks at 1
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "flan/flan.h"
#include "flanhip.h"

using namespace flan;

static int failures = 0;
#define CHECK( cond ) do { if( !( cond ) ) { std::printf( "FAILED: %s (line %d)\n", #cond, __LINE__ ); ++failures; } } while( 0 )

static Audio call( Second length, int fundamental_power, int spectrum_size_power, Channel ch, Second granularity, const std::vector<Radian> * phases = nullptr )
	{
	return Audio::synthesize_spectrum( length, 220.0f, []( Harmonic h ){ return Frequency( h ); }, []( Harmonic h ){ return 1.0f / std::sqrt( h ); },
		[]( Frequency x ){ return 1.0f / std::sqrt( pi2 ) * std::exp( -0.5f * std::pow( x, 2.0f ) ); }, fundamental_power, spectrum_size_power, ch, granularity, phases );
	}

static void null_checks()
	{
	CHECK( call( 0.0f, 8, 13, 2, 0.001f ).is_null() );                             // AudioSynthesis.cpp:163: length <= 0
	CHECK( call( -1.0f, 8, 13, 2, 0.001f ).is_null() );
	CHECK( call( 0.1f, 0, 13, 2, 0.001f ).is_null() );                             // :164
	CHECK( call( 0.1f, 8, 0, 2, 0.001f ).is_null() );                              // :165
	CHECK( call( 0.1f, 14, 13, 2, 0.001f ).is_null() );                            // :166
	CHECK( call( 0.1f, 8, 13, 2, 0.0f ).is_null() );                               // :167
	CHECK( call( 0.1f, 8, 13, 2, -0.5f ).is_null() );
	// sizes the library does not serve, a granularity below one frame, phases of the wrong length: null and a line on stderr
	CHECK( call( 0.1f, 4, 5, 2, 0.001f ).is_null() );
	CHECK( call( 0.1f, 8, 23, 2, 0.001f ).is_null() );
	CHECK( call( 0.1f, 8, 13, 2, 0.00001f ).is_null() );
	CHECK( call( 0.1f, 8, 13, 0, 0.001f ).is_null() );
	const std::vector<Radian> few( 100, 0.0f );
	CHECK( call( 0.1f, 8, 13, 2, 0.001f, &few ).is_null() );
	}

static void no_device_checks()
	{
	CHECK( call( 0.1f, 8, 13, 2, 0.001f ).is_null() );
	CHECK( Audio::synthesize_spectrum( 0.05f, []( Second t ){ return 200.0f + 100.0f * t; } ).is_null() );
	}

static float peak( const Audio & a )                                            // over the frames set_volume looks at: all but the last
	{
	float m = 0.0f;
	for( Channel c = 0; c < a.get_num_channels(); ++c )
		for( Frame f = 0; f + 1 < a.get_num_frames(); ++f ) m = std::max( m, std::fabs( a.get_sample_pointer( c, 0 )[f] ) );
	return m;
	}

static void device_checks()
	{
	const int cases[2][3] = { { 13, 8, 2 }, { 15, 6, 3 } };                        // spectrum_size_power, fundamental_power, channels
	for( const auto & k : cases )
		{
		const int p = k[0], fp = k[1], ch = k[2];
		const Frame n = 4800, g = 48;
		const int64_t bins = flanhip_spectrum_bins( p, fp, nullptr, nullptr, 0 );
		CHECK( bins == ( int64_t( 1 ) << ( p - 1 ) ) + 1 );
		std::vector<int32_t> harmonic( static_cast<size_t>( bins ) );
		std::vector<float> bin_frequency( harmonic.size() ), mag( harmonic.size() ), theta( harmonic.size() );
		flanhip_spectrum_bins( p, fp, harmonic.data(), bin_frequency.data(), bins );
		CHECK( flanhip_spectrum_phases( 4242u, harmonic.data(), bins, theta.data() ) == FLANHIP_OK );
		const float fundamental = float( 1 << fp );
		auto scale = []( Harmonic h ){ return 0.5f + 1.0f / float( h ); };
		auto sd = []( Harmonic h ){ return h == 2 ? 0.0005f : 3.0f + 0.25f * float( h ); };      // harmonic 2 takes the sd <= 0.001 branch
		auto dist = []( Frequency x ){ return 1.0f / ( 1.0f + x * x ); };
		for( int64_t b = 0; b < bins; ++b )
			{
			const int h = harmonic[size_t( b )];
			mag[size_t( b )] = 0.0f;
			if( h == 0 ) continue;
			const float x = bin_frequency[size_t( b )], mean = fundamental * h, s = sd( h );
			mag[size_t( b )] = ( s <= 0.001f ? x : dist( ( x - mean ) / s ) / s ) * scale( h );
			}
		// the frequency as the method samples it: at frame / 48000
		auto freq = []( Second t ){ return 180.0f + 400.0f * t; };
		std::vector<float> freq_v( static_cast<size_t>( n ) );
		for( Frame f = 0; f < n; ++f ) freq_v[size_t( f )] = freq( float( f ) / 48000.0f );
		std::vector<float> want( size_t( ch ) * size_t( n ) );
		CHECK( flanhip_audio_synthesize_spectrum( mag.data(), theta.data(), p, fp, ch, n, g, freq_v.data(), n, want.data(), nullptr ) == FLANHIP_OK );
		const Audio got = Audio::synthesize_spectrum( 0.1f, freq, sd, scale, dist, fp, p, ch, 0.001f, &theta );
		CHECK( !got.is_null() && got.get_num_frames() == n && got.get_num_channels() == ch && got.get_sample_rate() == 48000.0f );
		if( got.is_null() ) continue;
		CHECK( std::memcmp( want.data(), got.get_sample_pointer( 0, 0 ), sizeof( float ) * want.size() ) == 0 );
		std::printf( "p = %d: peak %.9g\n", p, peak( got ) );
		CHECK( std::fabs( peak( got ) - 1.0f ) <= 1.2e-7f );
		}
	// the defaults but for the length and the size: random phases, so two calls differ; each is normalised
	const Audio a = Audio::synthesize_spectrum( 0.05f, 220.0f, []( Harmonic h ){ return Frequency( h ); }, []( Harmonic h ){ return 1.0f / std::sqrt( h ); },
		[]( Frequency x ){ return 1.0f / std::sqrt( pi2 ) * std::exp( -0.5f * std::pow( x, 2.0f ) ); }, 8, 16 );
	const Audio b = Audio::synthesize_spectrum( 0.05f, 220.0f, []( Harmonic h ){ return Frequency( h ); }, []( Harmonic h ){ return 1.0f / std::sqrt( h ); },
		[]( Frequency x ){ return 1.0f / std::sqrt( pi2 ) * std::exp( -0.5f * std::pow( x, 2.0f ) ); }, 8, 16 );
	CHECK( !a.is_null() && !b.is_null() && a.get_num_frames() == 2400 && a.get_num_channels() == 2 );
	if( !a.is_null() && !b.is_null() )
		{
		CHECK( std::memcmp( a.get_sample_pointer( 0, 0 ), b.get_sample_pointer( 0, 0 ), sizeof( float ) * 4800 ) != 0 );
		CHECK( std::fabs( peak( a ) - 1.0f ) <= 1.2e-7f && std::fabs( peak( b ) - 1.0f ) <= 1.2e-7f );
		}
	}

int main( int argc, char ** argv )
	{
	const bool device = argc > 1 && std::strcmp( argv[1], "--device" ) == 0;
	null_checks();
	if( device )
		{
		if( flanhip_device_count() < 1 ) { std::printf( "FAILED: no device\n" ); return 1; }
		device_checks();
		}
	else if( flanhip_device_count() < 1 ) no_device_checks();
	if( failures ) { std::printf( "%d checks FAILED\n", failures ); return 1; }
	std::printf( "PASSED\n" );
	return 0;
	}
