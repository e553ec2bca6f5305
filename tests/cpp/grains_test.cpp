// grains_test.cpp -- Audio::cut, mix, join, synthesize_grains, texture, granulate and psola (include/flan/Audio.h, include/flan/AudioMod.h) over
// libflan_host.so.
//   grains_test --no-device          AudioMod; null and empty inputs; without a device the C ABI answers FLANHIP_ERR_NO_DEVICE and the methods
//                                    fail loudly with null Audios, while the host arithmetic works
//   grains_test --device             what can be said without a second opinion: identity mods, overloads against each other, scatter, nulls
//   grains_test --dump IN DIR        IN: raw fp32, two channels of equal length at 48 kHz, channel 0 a tone.  Runs the methods on it and writes
//                                    every result to DIR/<name>.bin (int32 channels, int32 frames, float sample rate, the samples) for the Python
//                                    suite, which computes the same with tests/grains_reference.py
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

static void mod_checks()
	{
	const AudioMod none;
	CHECK( none.is_null() );
	int calls = 0;
	const AudioMod some( [&calls]( Audio &, Second ){ ++calls; }, ExecutionPolicy::Linear_Sequenced );
	CHECK( !some.is_null() && some.get_execution_policy() == ExecutionPolicy::Linear_Sequenced );
	Audio a;
	some( a, 0.5f );
	none( a, 0.5f );
	CHECK( calls == 1 );
	const AudioMod moved( AudioMod( []( Audio &, Second ){} ) );
	CHECK( !moved.is_null() && moved.get_execution_policy() == ExecutionPolicy::Parallel_Unsequenced );
	static_assert( !std::is_copy_constructible_v<AudioMod> && std::is_move_constructible_v<AudioMod>, "move-only" );
	}

static void null_checks()
	{
	const Audio none;
	CHECK( none.cut( 0, 1 ).is_null() && none.cut_frames( 0, 10 ).is_null() );
	CHECK( Audio::mix( std::vector<const Audio *>{} ).is_null() );                // AudioCombination.cpp:109
	CHECK( Audio::mix( std::vector<const Audio *>{ nullptr } ).is_null() );
	CHECK( Audio::mix( std::vector<const Audio *>{ &none, &none } ).is_null() );  // nothing but null Audios
	CHECK( Audio::mix( std::vector<Audio>{} ).is_null() );
	CHECK( Audio::join( std::vector<const Audio *>{} ).is_null() );               // :210
	CHECK( none.texture( 1, 10, 0 ).is_null() && none.granulate( 1, 10, 0, 0, 0.1f ).is_null() && none.psola( 1, 0 ).is_null() );
	CHECK( Audio::synthesize_grains( 0, 10, 0, Function<Second, Audio>( []( Second ){ return Audio(); } ) ).is_null() );      // AudioSynthesis.cpp:385
	CHECK( Audio::synthesize_grains( 0.01f, 10, 0, Function<Second, Audio>( []( Second ){ return Audio(); } ) ).is_null() ); // only null grains
	}

static void host_checks( const Audio & a )
	{
	// what is decided before the device: end <= start, no frames after the clamp, times no frame holds, offsets of the wrong count
	CHECK( a.cut_frames( 10, 10 ).is_null() && a.cut_frames( 20, 10 ).is_null() && a.cut_frames( a.get_num_frames() + 5, a.get_num_frames() + 50 ).is_null() );
	CHECK( a.cut( 0.01f, INFINITY ).is_null() && a.cut( NAN, 0.01f ).is_null() && a.cut( 0.02f, 0.01f ).is_null() );
	CHECK( Audio::join( std::vector<const Audio *>{ &a, &a }, std::vector<Second>{ 0, 0 } ).is_null() );
	CHECK( a.texture( 0, 10, 0 ).is_null() && a.texture( -1, 10, 0 ).is_null() );
	CHECK( a.granulate( 0, 10, 0, 0, 0.1f ).is_null() );
	CHECK( a.granulate( 0.05f, 100, 0, 0.01f, -0.01f ).is_null() );               // every grain ends before it starts: nothing to mix
	}

static void no_device_checks()
	{
	const Audio a = Audio::create_from_buffer( noise( 4000, 3 ), 2, 48000.0f );
	host_checks( a );
	flanhip_grain_event e = {};
	e.src = uint64_t( 1 ) << 40; e.ch_stride = 2000; e.src_frames = 2000; e.n = 100; e.channels = 2; e.gain_offset = -1; e.gain = 1;
	int64_t frames = 0;
	int32_t first = 0, last = 0;
	CHECK( flanhip_grains_plan( &e, 1, &frames, nullptr, nullptr, 0 ) == FLANHIP_OK && frames == 100 );
	CHECK( flanhip_grains_plan( &e, 1, &frames, &first, &last, 1 ) == FLANHIP_OK && first == 0 && last == 0 );
	void * bogus = reinterpret_cast<void*>( uintptr_t( 1 ) << 41 );
	CHECK( flanhip_grains_mix_dev( &e, 1, &first, &last, 1, nullptr, 0, nullptr, 0, 2, 100, 48000.0f, static_cast<float*>( bogus ), bogus, nullptr ) == FLANHIP_ERR_NO_DEVICE );
	CHECK( a.cut( 0.0f, 0.01f ).is_null() && a.cut_frames( 0, 100 ).is_null() );
	CHECK( Audio::mix( a, a ).is_null() );
	CHECK( Audio::join( std::vector<const Audio *>{ &a, &a } ).is_null() );
	CHECK( a.texture( 0.01f, 1000, 0 ).is_null() );
	CHECK( a.granulate( 0.01f, 1000, 0, 0, 0.01f ).is_null() );
	}

static void device_checks()
	{
	const Frame n = 9000;
	const Audio a = Audio::create_from_buffer( noise( size_t( 2 * n ), 5 ), 2, 48000.0f );
	const Audio m = Audio::create_from_buffer( noise( 3000, 6 ), 1, 48000.0f );
	host_checks( a );
	// cut is cut_frames of the truncated times
	CHECK( same_bits( a.cut( 0.01f, 0.06f, 0.02f, 0.04f ), a.cut_frames( 480, 2880, 960, 1920 ) ) );
	const Audio whole = a.cut_frames( 0, n );
	CHECK( whole.get_num_frames() == n - 1 && whole.get_sample( 1, 77 ) == a.get_sample( 1, 77 ) );      // the end is clamped to n - 1
	// the overloads agree; constants as Functions are the constants
	const Function<Second, Amplitude> half( 0.5f ), one( 1.0f );
	const Audio by_values = Audio::mix( std::vector<const Audio *>{ &a, &m }, std::vector<Second>{ 0.01f, 0.0f }, std::vector<Amplitude>{ 0.5f, 1.0f } );
	CHECK( !by_values.is_null() && by_values.get_num_channels() == 2 && by_values.get_num_frames() == n + 480 );
	CHECK( same_bits( by_values, Audio::mix( std::vector<const Audio *>{ &a, &m }, std::vector<Second>{ 0.01f, 0.0f }, std::vector<const Function<Second, Amplitude> *>{ &half, &one } ) ) );
	CHECK( same_bits( by_values, Audio::mix( std::vector<const Audio *>{ &a, &m }, std::vector<Second>{ 0.01f }, std::vector<Amplitude>{ 0.5f } ) ) );       // short lists: 0 and 1
	std::vector<Audio> owned;
	owned.emplace_back( a.copy() ); owned.emplace_back( m.copy() );
	CHECK( same_bits( by_values, Audio::mix( owned, std::vector<Second>{ 0.01f, 0.0f }, std::vector<Amplitude>{ 0.5f, 1.0f } ) ) );
	CHECK( same_bits( Audio::mix( a, m ), Audio::mix( std::vector<const Audio *>{ &a, &m } ) ) );
	// a callable amplitude that returns the constant gives the constant's bits
	const Function<Second, Amplitude> half_fn( []( Second ){ return 0.5f; } );
	CHECK( same_bits( by_values, Audio::mix( std::vector<const Audio *>{ &a, &m }, std::vector<Second>{ 0.01f, 0.0f }, std::vector<const Function<Second, Amplitude> *>{ &half_fn, &one } ) ) );
	// a null Audio among the inputs counts for the length alone
	const Audio none;
	const Audio with_null = Audio::mix( std::vector<const Audio *>{ &m, &none }, std::vector<Second>{ 0.0f, 0.5f } );
	CHECK( with_null.get_num_frames() == 24000 && with_null.get_sample( 0, 100 ) == m.get_sample( 0, 100 ) && with_null.get_sample( 0, 23999 ) == 0 );
	// join is mix at the running ends
	const Audio joined = Audio::join( std::vector<const Audio *>{ &m, &a, &m }, 0.01f );
	CHECK( same_bits( joined, Audio::mix( std::vector<const Audio *>{ &m, &a, &m }, std::vector<Second>{ 0.0f, m.get_length() + 0.01f, ( m.get_length() + 0.01f ) + a.get_length() + 0.01f } ) ) );
	// granulate: an identity mod takes the general path and gives the null mod's bits
	const Function<Second, Second> selection( []( Second t ){ return 0.02f + 0.4f * t; } ), length( []( Second t ){ return 0.004f + 0.05f * t; } );
	const Audio fused = a.granulate( 0.15f, 800.0f, 0.0f, selection, length, 0.003f );
	int calls = 0;
	const Audio general = a.granulate( 0.15f, 800.0f, 0.0f, selection, length, 0.003f, AudioMod( [&calls]( Audio &, Second ){ ++calls; } ) );
	CHECK( !fused.is_null() && fused.get_num_channels() == 2 && calls == 120 );
	CHECK( same_bits( fused, general ) );
	// texture: an identity mod gives the null mod's bits, with and without feedback
	const Audio repeated = m.texture( 0.2f, 50.0f, 0.0f );
	CHECK( !repeated.is_null() && repeated.get_num_frames() == 8640 + 3000 );    // events at 0, 960, 1920, ... 8640
	CHECK( same_bits( repeated, m.texture( 0.2f, 50.0f, 0.0f, AudioMod( []( Audio &, Second ){} ) ) ) );
	CHECK( same_bits( repeated, m.texture( 0.2f, 50.0f, 0.0f, AudioMod( []( Audio &, Second ){} ), true ) ) );
	// scatter: events move, the result stays inside length + the source
	const Audio scattered = m.texture( 0.2f, 50.0f, 0.3f );
	CHECK( !scattered.is_null() && scattered.get_num_frames() <= 9600 + 3000 && scattered.get_num_frames() > 3000 );
	// synthesize_grains with the caller's grains is mix at the event times
	const Audio grains = Audio::synthesize_grains( 0.2f, 50.0f, 0.0f, Function<Second, Audio>( [&m]( Second ){ return m.copy(); } ) );
	CHECK( same_bits( grains, repeated ) );
	// psola: an identity mod gives a result of the same shape within the device cos' last places of the fused one
	std::vector<float> tone( 12000 );
	for( size_t i = 0; i < tone.size(); ++i ) tone[i] = float( 0.4 * std::sin( 6.283185307179586 * 220.0 * double( i ) / 48000.0 ) + 0.2 * std::sin( 6.283185307179586 * 440.0 * double( i ) / 48000.0 ) )
		+ 0.01f * noise( 1, uint32_t( i ) )[0];
	const Audio voiced = Audio::create_from_buffer( std::move( tone ), 1, 48000.0f );
	const Function<Second, Second> same_time( []( Second t ){ return t; } );
	const Audio p_fused = voiced.psola( 0.2f, same_time ), p_general = voiced.psola( 0.2f, same_time, AudioMod( []( Audio &, Second ){} ) );
	CHECK( !p_fused.is_null() && !p_general.is_null() && p_fused.get_num_frames() == p_general.get_num_frames() );
	if( !p_fused.is_null() && p_fused.get_num_frames() == p_general.get_num_frames() )
		{
		float worst = 0, peak = 0;
		for( Frame f = 0; f < p_fused.get_num_frames(); ++f )
			{
			worst = std::max( worst, std::fabs( p_fused.get_sample( 0, f ) - p_general.get_sample( 0, f ) ) );
			peak = std::max( peak, std::fabs( p_fused.get_sample( 0, f ) ) );
			}
		std::printf( "psola fused against general: largest difference %.3g under a peak of %.3g\n", worst, peak );
		CHECK( peak > 0.1f && worst <= 4e-7f * peak * 4 );                        // a few fp32 spacings of the sum: only the cos may differ
		}
	}

static bool write_audio( const std::string & dir, const char * name, const Audio & a )
	{
	std::FILE * out = std::fopen( ( dir + "/" + name + ".bin" ).c_str(), "wb" );
	if( !out ) { std::printf( "FAILED: cannot write %s\n", name ); return false; }
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
	const Frame n = Frame( x.size() / 2 );
	const Audio S = Audio::create_from_buffer( std::vector<float>( x ), 2, 48000.0f );                                 // stereo
	const Audio P = Audio::create_from_buffer( std::vector<float>( x.begin(), x.begin() + n ), 1, 48000.0f );           // the tone, mono
	const Audio M = Audio::create_from_buffer( std::vector<float>( x.begin(), x.begin() + 5000 ), 1, 48000.0f );       // its first 5000 frames
	const Audio R = Audio::create_from_buffer( std::vector<float>( x.begin() + n, x.begin() + n + 3000 ), 1, 44100.0f ); // another rate
	bool ok = true;
	const auto put = [&]( const char * name, const Audio & a ){ ok = write_audio( dir, name, a ) && ok; };
	const Function<Second, Amplitude> ramp( []( Second t ){ return 0.25f + 2.0f * t; } ), level( -0.75f );

	put( "cut", S.cut( 0.01f, 0.06f, 0.02f, 0.04f ) );
	put( "cut_frames", S.cut_frames( -5, 3000, 4000, 100 ) );
	put( "mix_short", Audio::mix( std::vector<const Audio *>{ &S, &M }, std::vector<Second>{ 0.01f, 0.0f, 0.05f }, std::vector<Amplitude>{ 0.5f } ) );
	{
	std::vector<Audio> owned;
	owned.emplace_back( S.copy() ); owned.emplace_back( M.copy() );
	put( "mix_values", Audio::mix( owned, std::vector<Second>{ 0.0f, 0.02f }, std::vector<Amplitude>{ 1.0f, -2.0f } ) );
	std::vector<Function<Second, Amplitude>> amps;
	amps.emplace_back( []( Second t ){ return 0.25f + 2.0f * t; } ); amps.emplace_back( -0.75f );
	put( "mix_functions_values", Audio::mix( owned, std::vector<Second>{ 0.03f, 0.0f }, amps ) );
	put( "join_values", Audio::join( owned, -0.005f ) );
	}
	put( "mix_functions", Audio::mix( std::vector<const Audio *>{ &S, &M, &M }, std::vector<Second>{ 0.03f, 0.0f, -0.01f }, std::vector<const Function<Second, Amplitude> *>{ &ramp, &level, &ramp } ) );
	put( "mix_variadic", Audio::mix( S, M, M ) );
	put( "r48", R.resample( 48000.0f ) );
	put( "mix_rates", Audio::mix( std::vector<const Audio *>{ &R, &M }, std::vector<Second>{ 0.0f, 0.01f } ) );
	put( "join", Audio::join( std::vector<const Audio *>{ &M, &S, &M }, 0.01f ) );
	put( "join_offsets", Audio::join( std::vector<const Audio *>{ &M, &S, &M }, std::vector<Second>{ 9.0f, 0.02f, -0.01f, 9.0f } ) );
	put( "texture", S.texture( 0.1f, 200.0f, 0.0f ) );
	put( "texture_mod", M.texture( 0.1f, 200.0f, 0.0f, AudioMod( []( Audio & a, Second t ){ a.modify_volume_in_place( 0.5f + t ); } ) ) );
	put( "texture_feedback", M.texture( 0.1f, 200.0f, 0.0f, AudioMod( []( Audio & a, Second ){ a.modify_volume_in_place( 0.9f ); } ), true ) );
	const Function<Second, Second> selection( []( Second t ){ return 0.05f + 0.3f * t; } ), length( []( Second t ){ return 0.01f + 0.1f * t; } );
	const Function<Second, float> rate( []( Second t ){ return 300.0f + 2000.0f * t; } );
	put( "granulate", S.granulate( 0.2f, rate, 0.0f, selection, length, 0.004f ) );
	put( "granulate_identity", S.granulate( 0.2f, rate, 0.0f, selection, length, 0.004f, AudioMod( []( Audio &, Second ){} ) ) );
	put( "granulate_mod", S.granulate( 0.2f, rate, 0.0f, selection, length, 0.004f, AudioMod( []( Audio & a, Second ){ a.modify_volume_in_place( 0.5f ); } ) ) );
	put( "psola_1", P.psola( P.get_length(), Function<Second, Second>( []( Second t ){ return t; } ) ) );
	put( "psola_2", P.psola( 2.0f * P.get_length(), Function<Second, Second>( []( Second t ){ return t / 2.0f; } ) ) );
	put( "psola_mod", P.psola( 0.1f, Function<Second, Second>( []( Second t ){ return 0.1f + t; } ), AudioMod( []( Audio &, Second ){} ) ) );
	return ok ? 0 : 1;
	}

int main( int argc, char ** argv )
	{
	const char * mode = argc > 1 ? argv[1] : "--no-device";
	std::ostringstream captured;                                               // "Null Audio created"
	std::streambuf * old = std::cout.rdbuf( captured.rdbuf() );
	mod_checks();
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
