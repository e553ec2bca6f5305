// temporal_test.cpp -- Audio::get_loud_chunks, remove_silence, remove_edge_silence, reverse, modify_boundaries, the splits, rearrange, random_chunks,
// iterate and delay (include/flan/Audio.h) over libflan_host.so.
//   temporal_test --no-device        null inputs; without a device the C ABI answers FLANHIP_ERR_NO_DEVICE and the methods fail loudly with null
//                                    Audios and empty vectors, while the host arithmetic works
//   temporal_test --device           what can be said without a second opinion: fused against general paths, seeds, nulls, nothing noisy
//   temporal_test --dump IN DIR      IN: raw fp32, two channels of equal length at 48 kHz, gated bursts.  Runs the methods on it and writes every
//                                    result to DIR/<name>.bin (int32 channels, int32 frames, float sample rate, the samples) for the Python
//                                    suite, which computes the same with tests/temporal_reference.py
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

static const float LEVEL = 0.2f, GAP = 50.0f / 48000.0f;

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

// two channels of n frames: bursts of noise (channel 0 always above LEVEL inside one) between silences
static Audio gated( Frame n, uint32_t seed )
	{
	std::vector<float> v = noise( size_t( 2 * n ), seed );
	for( Frame f = 0; f < n; ++f )
		{
		const bool burst = ( f % 1000 ) >= 150 && ( f % 1000 ) < 700;
		v[size_t( f )] = burst ? 0.7f + 0.3f * v[size_t( f )] : 0.0f;
		v[size_t( n + f )] = burst ? v[size_t( n + f )] : 0.0f;
		}
	return Audio::create_from_buffer( std::move( v ), 2, 48000.0f );
	}

static void null_checks()
	{
	const Audio none;
	CHECK( none.get_loud_chunks( LEVEL, GAP ).empty() && none.remove_silence( LEVEL, GAP ).is_null() && none.remove_silence_unfused( LEVEL, GAP ).is_null() );
	CHECK( none.remove_edge_silence( LEVEL ).is_null() && none.reverse().is_null() );
	CHECK( none.modify_boundaries_frames( -10, 10 ).is_null() && none.modify_boundaries( -0.1f, 0.1f ).is_null() );
	CHECK( none.split_at_times( { 0.1f } ).empty() && none.split_with_lengths( { 0.1f } ).empty() && none.split_with_equal_lengths( 0.1f ).empty() );
	CHECK( none.rearrange( 0.1f, 0, 1 ).is_null() && none.random_chunks( 1, 0.1f, 0, AudioMod(), 1 ).is_null() );
	CHECK( none.iterate( 3 ).is_null() && none.delay( 1, 0.1f ).is_null() );
	}

// what is decided before the device
static void host_checks( const Audio & a )
	{
	CHECK( a.modify_boundaries_frames( a.get_num_frames(), 0 ).is_null() && a.modify_boundaries_frames( 10, -a.get_num_frames() ).is_null() );      // <= 0 frames
	CHECK( a.iterate( 0 ).is_null() && a.iterate( -3 ).is_null() );
	CHECK( a.split_with_equal_lengths( 0 ).empty() && a.split_with_equal_lengths( -1 ).empty() );
	CHECK( a.random_chunks( 0, 0.1f, 0, AudioMod(), 1 ).is_null() && a.random_chunks( -1, 0.1f, 0, AudioMod(), 1 ).is_null() );
	CHECK( a.rearrange( a.get_length() * 2, 0, 1 ).is_null() );                   // one piece
	CHECK( a.get_loud_chunks( LEVEL, INFINITY ).empty() );                        // a gap no frame holds
	int32_t order[5] = { 0, 0, 0, 0, 0 }, again[5];
	CHECK( flanhip_rearrange_order( 5, 7, order ) == FLANHIP_OK && flanhip_rearrange_order( 5, 7, again ) == FLANHIP_OK && !std::memcmp( order, again, sizeof( order ) ) );
	std::sort( again, again + 5 );
	for( int i = 0; i < 5; ++i ) CHECK( again[i] == i );
	}

static void no_device_checks()
	{
	const Audio a = gated( 3000, 3 );
	host_checks( a );
	void * bogus = reinterpret_cast<void*>( uintptr_t( 1 ) << 41 );
	CHECK( flanhip_loud_summary_dev( static_cast<float*>( bogus ), 2, 3000, LEVEL, 50, static_cast<int64_t*>( bogus ), bogus, nullptr ) == FLANHIP_ERR_NO_DEVICE );
	CHECK( flanhip_audio_reverse_dev( static_cast<float*>( bogus ), 2, 3000, static_cast<float*>( bogus ) + 8000, nullptr ) == FLANHIP_ERR_NO_DEVICE );
	CHECK( a.get_loud_chunks( LEVEL, GAP ).empty() && a.remove_silence( LEVEL, GAP ).is_null() && a.remove_silence_unfused( LEVEL, GAP ).is_null() );
	CHECK( a.remove_edge_silence( LEVEL ).is_null() && a.reverse().is_null() && a.modify_boundaries_frames( -10, 10 ).is_null() );
	const std::vector<Audio> pieces = a.split_with_equal_lengths( 0.02f );
	CHECK( pieces.size() == 4 );                                                   // the plan is host work; every piece is a null Audio
	for( const Audio & p : pieces ) CHECK( p.is_null() );
	CHECK( a.rearrange( 0.01f, 0, 1 ).is_null() && a.random_chunks( 0.05f, 0.01f, 0, AudioMod(), 1 ).is_null() );
	CHECK( a.iterate( 2 ).is_null() && a.delay( 0.01f, 0.01f ).is_null() );
	}

// rearrange's general path from public pieces: the slices made, permuted by the library's own order, joined
static Audio rearrange_general( const Audio & a, Second slice, Second fade, uint64_t seed )
	{
	std::vector<Audio> chops = a.split_with_equal_lengths( slice + fade, fade );
	if( chops.size() < 2 ) return Audio();
	chops.pop_back();
	std::vector<int32_t> order( chops.size() );
	if( flanhip_rearrange_order( int64_t( order.size() ), seed, order.data() ) != FLANHIP_OK ) return Audio();
	std::vector<const Audio *> picked;
	for( int32_t p : order ) picked.push_back( &chops[size_t( p )] );
	return Audio::join( picked, -fade );
	}

static void device_checks()
	{
	const Frame n = 6000;
	const Audio a = gated( n, 5 );
	host_checks( a );
	// remove_silence: one launch over *this against the chunks made and joined
	for( float fade : { 0.0f, 0.001f, 0.05f } )
		{
		const Audio fused = a.remove_silence( LEVEL, GAP, fade );
		CHECK( !fused.is_null() && fused.get_num_channels() == 2 );
		CHECK( same_bits( fused, a.remove_silence_unfused( LEVEL, GAP, fade ) ) );
		}
	const std::vector<Audio> chunks = a.get_loud_chunks( LEVEL, GAP );
	CHECK( chunks.size() == 6 );
	if( chunks.size() == 6 ) CHECK( chunks[0].get_num_frames() == 549 && chunks[0].get_sample( 0, 0 ) == a.get_sample( 0, 150 ) );      // { 150, 699 }: the end is the last noisy frame
	// a one-frame chunk with no fade cuts to nothing: an empty event on the fused path, a null Audio among join's inputs on the general one
	{
	std::vector<float> v( 4000, 0.0f );
	v[100] = 1.0f;
	for( size_t f = 1000; f < 1200; ++f ) v[f] = 0.5f;
	v[2000 + 1900] = 0.9f;                                                        // channel 1, frame 1900
	const Audio lone = Audio::create_from_buffer( std::move( v ), 2, 48000.0f );
	const std::vector<Audio> parts = lone.get_loud_chunks( LEVEL, GAP );
	CHECK( parts.size() == 3 && parts[0].is_null() && !parts[1].is_null() && parts[2].is_null() );
	CHECK( same_bits( lone.remove_silence( LEVEL, GAP ), lone.remove_silence_unfused( LEVEL, GAP ) ) );
	CHECK( same_bits( lone.remove_silence( LEVEL, GAP, 0.002f ), lone.remove_silence_unfused( LEVEL, GAP, 0.002f ) ) );
	}
	// nothing noisy
	const Audio quiet = Audio::create_empty_with_frames( 5000, 2, 48000.0f );
	CHECK( quiet.get_loud_chunks( LEVEL, GAP ).empty() && quiet.remove_silence( LEVEL, GAP ).is_null() && quiet.remove_edge_silence( LEVEL ).is_null() );
	CHECK( quiet.get_loud_chunks( -1.0f, GAP ).size() == 1 );                     // a negative level: every frame is noisy
	// edges: the first and the last noisy frame
	const Audio trimmed = a.remove_edge_silence( LEVEL );
	CHECK( same_bits( trimmed, a.cut_frames( 150, 5700 ) ) );
	// reverse twice is the identity
	CHECK( same_bits( a.reverse().reverse(), a ) && a.reverse().get_sample( 1, 0 ) == a.get_sample( 1, n - 1 ) );
	// boundaries: padding then cutting it off again
	const Audio padded = a.modify_boundaries_frames( -100, 50 );
	CHECK( padded.get_num_frames() == n + 150 && padded.get_sample( 0, 99 ) == 0 && padded.get_sample( 0, 100 + 200 ) == a.get_sample( 0, 200 ) && padded.get_sample( 1, n + 120 ) == 0 );
	CHECK( same_bits( padded.modify_boundaries_frames( 100, -50 ), a ) );
	CHECK( a.modify_boundaries_frames( 5000, -2000 ).is_null() );
	// the splits agree with one another
	const std::vector<Audio> by_times = a.split_at_times( { 0.08f, 0.02f, 0.06f, 0.04f, 0.1f, 0.12f }, 0.001f ), by_lengths = a.split_with_lengths( std::vector<Second>( 7, 0.02f ), 0.001f ),
		by_equal = a.split_with_equal_lengths( 0.02f, 0.001f );
	CHECK( by_times.size() == 7 && by_lengths.size() == 7 && by_equal.size() == 7 );
	if( by_times.size() == 7 ) CHECK( same_bits( by_times[0], a.cut_frames( 0, 960, 48, 48 ) ) );
	for( size_t i = 0; i < by_equal.size() && i < by_lengths.size(); ++i ) CHECK( same_bits( by_equal[i], by_lengths[i] ) );
	// rearrange: a seed names one result; fused equals general; another seed another order
	const Audio r1 = a.rearrange( 0.01f, 0.002f, 11 );
	CHECK( !r1.is_null() && same_bits( r1, a.rearrange( 0.01f, 0.002f, 11 ) ) && same_bits( r1, rearrange_general( a, 0.01f, 0.002f, 11 ) ) );
	CHECK( !same_bits( r1, a.rearrange( 0.01f, 0.002f, 12 ) ) );
	// random_chunks: the same, with an identity mod for the general path
	const Function<Second, Second> lengths( []( Second t ){ return 0.005f + 0.05f * t; } ), fades( []( Second t ){ return 0.001f + 0.01f * t; } );
	const Audio c1 = a.random_chunks( 0.1f, lengths, fades, AudioMod(), 5 );
	int calls = 0;
	CHECK( !c1.is_null() && same_bits( c1, a.random_chunks( 0.1f, lengths, fades, AudioMod(), 5 ) ) );
	CHECK( same_bits( c1, a.random_chunks( 0.1f, lengths, fades, AudioMod( [&calls]( Audio &, Second ){ ++calls; } ), 5 ) ) && calls > 3 );
	CHECK( !same_bits( c1, a.random_chunks( 0.1f, lengths, fades, AudioMod(), 6 ) ) );
	// iterate without a mod is join of pointers to *this; an identity mod gives the same bits
	const Audio thrice = a.iterate( 3, 0.01f );
	CHECK( same_bits( thrice, Audio::join( std::vector<const Audio *>( 3, &a ), -0.01f ) ) );
	CHECK( same_bits( thrice, a.iterate( 3, 0.01f, AudioMod( []( Audio &, Second ){} ) ) ) && same_bits( thrice, a.iterate( 3, 0.01f, AudioMod( []( Audio &, Second ){} ), true ) ) );
	// delay: a decay of 1 is texture at the delay's rate
	const Audio echoed = a.delay( 0.05f, 0.02f, 1.0f );
	CHECK( !echoed.is_null() && same_bits( echoed, a.texture( a.get_length() + 0.05f, 1.0f / 0.02f, 0.0f ) ) );
	std::printf( "temporal methods on the device\n" );
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
	const Audio S = Audio::create_from_buffer( std::vector<float>( x ), 2, 48000.0f );
	bool ok = true;
	const auto put = [&]( const std::string & name, const Audio & a ){ ok = write_audio( dir, name, a ) && ok; };
	const auto put_all = [&]( const std::string & name, const std::vector<Audio> & v ){ for( size_t i = 0; i < v.size(); ++i ) put( name + "_" + std::to_string( i ), v[i] ); };

	const float fades[3] = { 0.0f, 0.001f, 0.05f };
	for( int k = 0; k < 3; ++k )
		{
		const std::string tag = std::to_string( k );
		put( "rs_fused_" + tag, S.remove_silence( LEVEL, GAP, fades[k] ) );
		put( "rs_general_" + tag, S.remove_silence_unfused( LEVEL, GAP, fades[k] ) );
		put_all( "chunks_" + tag, S.get_loud_chunks( LEVEL, GAP, fades[k] ) );
		put( "edge_" + tag, S.remove_edge_silence( LEVEL, fades[k] ) );
		}
	for( Frame n : { 1, 2, 4095, 4097 } )                                          // three rows, so rows 1 and 2 start off a 16-byte boundary
		put( "reverse_" + std::to_string( n ), Audio::create_from_buffer( std::vector<float>( x.begin(), x.begin() + 3 * n ), 3, 48000.0f ).reverse() );
	put( "mb_pad", S.modify_boundaries_frames( -100, 50 ) );
	put( "mb_cut", S.modify_boundaries_frames( 200, -300 ) );
	put( "mb_pad_cut", S.modify_boundaries_frames( -37, -41 ) );
	put( "mb_cut_pad", S.modify_boundaries_frames( 64, 10 ) );
	put( "mb_times", S.modify_boundaries( -0.01f, 0.02f ) );
	put_all( "split_times", S.split_at_times( { 0.05f, 0.01f, -1.0f, 0.08f, 9.0f }, 0.002f ) );
	put_all( "split_lengths", S.split_with_lengths( { 0.02f, -1.0f, 0.03f, 0.01f }, 0.0f ) );
	put_all( "split_equal", S.split_with_equal_lengths( 0.03f, 0.001f ) );
	put( "rearrange", S.rearrange( 0.01f, 0.002f, 11 ) );
	const Function<Second, Second> lengths( []( Second t ){ return 0.005f + 0.05f * t; } ), fade( []( Second t ){ return 0.001f + 0.01f * t; } );
	put( "random_chunks", S.random_chunks( 0.1f, lengths, fade, AudioMod(), 5 ) );
	put( "random_chunks_mod", S.random_chunks( 0.1f, lengths, fade, AudioMod( []( Audio & a, Second t ){ a.modify_volume_in_place( 0.5f + t ); } ), 5 ) );
	put( "iterate", S.iterate( 3, 0.01f ) );
	put( "iterate_feedback", S.iterate( 3, 0.0f, AudioMod( []( Audio & a, Second ){ a.modify_volume_in_place( 0.5f ); } ), true ) );
	put( "delay_constant", S.delay( 0.05f, 0.02f, 0.5f ) );
	put( "delay_ramped", S.delay( 0.03f, Function<Second, Second>( []( Second t ){ return 0.01f + 0.1f * t; } ), Function<Second, float>( []( Second t ){ return 0.8f - t; } ) ) );
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
