// temporal.hip -- the loud-chunk detection under Audio::get_loud_chunks, remove_silence and remove_edge_silence (Audio/AudioTemporal.cpp:10-86,
// 124-172), Audio::reverse (:174-188), and the host arithmetic of the slicing family (:52-83, :149-152, :409-533).  DESIGN.md section 4.25.
//
// The reference finds the chunks with one sequential loop over all frames (:20-48): a frame is NOISY when some channel's sample is above the
// level (signed, no abs; a NaN never is); a chunk opens at a noisy frame met in a quiet sector and closes once more than `gap` frames have
// passed since the last noisy one, with that frame as its end; a chunk still open after the last frame ends at num_frames.  That loop is a
// scan of a small associative map over the frames:
//   a map is EMPTY or ( first, last, inner ): the first and the last noisy frame and the chunk starts other than `first`
//   then( a, b ) = a if b is EMPTY, b if a is EMPTY, else ( a.first, b.last, a.inner + b.inner + ( b.first - a.last > gap + 1 ) )
// A noisy frame f with exclusive prefix P starts a chunk iff P is EMPTY or f - P.last > gap + 1; it is chunk P.inner + 1 (0 if P is EMPTY)
// and closes the chunk before it with end P.last.  then() must not see gap (run_scan.h finds it by its two arguments), so a map carries
// reach = last + gap + 1 clamped into an int beside last, and the test is b.first > a.reach.  first is kept as first + 1 so that the
// all-zero object -- k_scan_carry's S{} -- is EMPTY.
//   k_loud_sum      a lane owns a run of frames: reads every channel's run once, leaves the run's noisy bits as one 64-bit mask in the
//                   workspace, reduces them to one map, block_scan, the block's total
//   k_scan_carry    run_scan.h's, over the block totals: the map of everything before each block
//   k_loud_close    one thread: the summary { count, first, last, 0 } from the last block's carry and total
//   k_loud_chunks   the block's lane maps again from the masks (no audio is read), block_scan, each lane walks its mask from the carried
//                   prefix and writes chunks[k] = { start, end }; the last block's first thread writes the last chunk's end
// Every int of the table has exactly one writer: plain stores, no atomics.  The geometry, block_scan, load4, lane_run and k_scan_carry are
// run_scan.h's.
#include "run_scan.h"

#include <climits>
#include <cstring>
#include <random>

namespace flanhip {

namespace {

thread_local int t_loud_run = 0;          // flanhip_loud_debug_run: frames per lane forced for the calling thread (0: the library's choice)

constexpr int64_t LOUD_MAX_CHANNELS = 1 << 20;

struct LoudMap { int first1, last, reach, inner; };     // first1 = first + 1; 0: EMPTY

struct LoudLayout
	{
	int run = 0;
	int64_t blocks = 0;
	size_t tot = 0, carry = 0, masks = 0, total = 0;
	};

bool loud_layout( int64_t ch, int64_t n, LoudLayout * l )
	{
	if( ch <= 0 || ch > LOUD_MAX_CHANNELS || n <= 0 || n > INT32_MAX ) return false;
	const auto up = []( size_t v ){ return ( v + 255 ) & ~size_t( 255 ); };
	l->run = scan_run( t_loud_run );
	l->blocks = scan_blocks( n, l->run );
	l->tot = 0;
	l->carry = l->tot + up( sizeof( LoudMap ) * size_t( l->blocks ) );
	l->masks = l->carry + up( sizeof( LoudMap ) * size_t( l->blocks ) );
	l->total = l->masks + up( sizeof( uint64_t ) * size_t( l->blocks ) * SCAN_THREADS );
	return true;
	}

// ---- the map ----------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void set_identity( LoudMap & m ) { m = LoudMap{ 0, 0, 0, 0 }; }
__device__ __forceinline__ LoudMap then( const LoudMap & e, const LoudMap & l )
	{
	if( l.first1 == 0 ) return e;
	if( e.first1 == 0 ) return l;
	return LoudMap{ e.first1, l.last, l.reach, e.inner + l.inner + ( l.first1 - 1 > e.reach ? 1 : 0 ) };
	}
__device__ __forceinline__ LoudMap apply( const LoudMap & m, const LoudMap & state ) { return then( state, m ); }
__device__ __forceinline__ LoudMap shfl_up( const LoudMap & m, int off )
	{
	return LoudMap{ __shfl_up( m.first1, off ), __shfl_up( m.last, off ), __shfl_up( m.reach, off ), __shfl_up( m.inner, off ) };
	}
// the last frame a noisy frame f keeps its chunk open for a next noisy one: f + gap + 1, held in an int (frames are below INT_MAX, so
// INT_MAX is never exceeded by one, and -1 by every one)
__device__ __forceinline__ int reach_of( int64_t f, int64_t gap )
	{
	const int64_t r = f + gap + 1;
	return int( r < -1 ? -1 : r > INT_MAX ? INT_MAX : r );
	}
// the map `p` followed by the noisy frame f; starts: f opens a chunk
__device__ __forceinline__ void step( LoudMap & p, int64_t f, int64_t gap, bool & starts )
	{
	starts = p.first1 == 0 || f > p.reach;
	if( p.first1 == 0 ) { p.first1 = int( f ) + 1; p.inner = 0; }
	else if( starts ) p.inner += 1;
	p.last = int( f );
	p.reach = reach_of( f, gap );
	}
// a run's mask (bit i: frame f0 + i is noisy) as one map
__device__ __forceinline__ LoudMap map_of_mask( uint64_t mask, int64_t f0, int64_t gap )
	{
	LoudMap m; set_identity( m );
	while( mask )
		{
		const int i = __ffsll( (unsigned long long) mask ) - 1;
		mask &= mask - 1;
		bool starts;
		step( m, f0 + i, gap, starts );
		}
	return m;
	}

// ---- kernels ----------------------------------------------------------------------------------------------------------------------
// VEC: run a multiple of 4, n a multiple of 4 and the audio 16-byte aligned: every quad of every channel's row is aligned and whole
template<bool VEC>
__global__ __launch_bounds__( SCAN_THREADS ) void k_loud_sum( const float * __restrict__ audio, int64_t ch, int64_t n, float level, int64_t gap, int run,
	LoudMap * __restrict__ tot, uint64_t * __restrict__ masks )
	{
	__shared__ LoudMap s_tot[SCAN_WAVES];
	int64_t f0; int len;
	lane_run( n, run, f0, len );
	uint64_t mask = 0;
	for( int64_t c = 0; c < ch; ++c )
		{
		const float * row = audio + c * n;
		for( int i = 0; i < len; i += 4 )
			{
			float v[4];
			load4<VEC>( row, f0 + i, len - i, v );
			#pragma unroll
			for( int k = 0; k < 4; ++k )
				if( i + k < len && v[k] > level ) mask |= uint64_t( 1 ) << ( i + k );      // :29: signed, and false for a NaN
			}
		}
	masks[int64_t( blockIdx.x ) * SCAN_THREADS + threadIdx.x] = mask;
	LoudMap excl, total;
	block_scan( map_of_mask( mask, f0, gap ), s_tot, excl, total );
	if( threadIdx.x == 0 ) tot[blockIdx.x] = total;
	}

// { count, first noisy frame, last noisy frame, 0 }; -1 for the frames when nothing is noisy
__global__ void k_loud_close( const LoudMap * __restrict__ tot, const LoudMap * __restrict__ carry, int64_t blocks, int64_t * __restrict__ summary )
	{
	if( blockIdx.x != 0 || threadIdx.x != 0 ) return;
	const LoudMap all = then( carry[blocks - 1], tot[blocks - 1] );
	summary[0] = all.first1 == 0 ? 0 : int64_t( all.inner ) + 1;
	summary[1] = int64_t( all.first1 ) - 1;
	summary[2] = all.first1 == 0 ? -1 : int64_t( all.last );
	summary[3] = 0;
	}

// chunks: int[count][2], count the chunk count the caller read from the summary.  Nothing is written at or past `count`
__global__ __launch_bounds__( SCAN_THREADS ) void k_loud_chunks( const uint64_t * __restrict__ masks, const LoudMap * __restrict__ carry, int64_t n, int64_t gap,
	int run, int * __restrict__ chunks, int64_t count )
	{
	__shared__ LoudMap s_tot[SCAN_WAVES];
	int64_t f0; int len;
	lane_run( n, run, f0, len );
	uint64_t mask = masks[int64_t( blockIdx.x ) * SCAN_THREADS + threadIdx.x];
	LoudMap excl, total;
	block_scan( map_of_mask( mask, f0, gap ), s_tot, excl, total );
	const LoudMap before = carry[blockIdx.x];
	LoudMap p = then( before, excl );
	while( mask )
		{
		const int i = __ffsll( (unsigned long long) mask ) - 1;
		mask &= mask - 1;
		const LoudMap was = p;
		bool starts;
		step( p, f0 + i, gap, starts );
		if( !starts ) continue;
		const int64_t k = p.inner;                                   // 0 for the first chunk of all, else was.inner + 1
		if( k < count ) chunks[2 * k] = int( f0 + i );
		if( k > 0 && k - 1 < count ) chunks[2 * ( k - 1 ) + 1] = was.last;       // :44: the chunk before ends at its last noisy frame
		}
	if( blockIdx.x == gridDim.x - 1 && threadIdx.x == 0 )
		{
		const LoudMap all = then( before, total );
		if( all.first1 != 0 && int64_t( all.inner ) < count )      // :47-48: still open after the last frame: it ends at num_frames
			chunks[2 * int64_t( all.inner ) + 1] = int64_t( all.last ) + gap + 1 < n ? all.last : int( n );
		}
	}

// out[c][f] = in[c][n - 1 - f].  A block's threads own consecutive quads of one row's output, cut at the 16-byte boundaries of the OUTPUT
// (a row starts wherever c * n puts it): frames [head + 4 q, head + 4 q + 4); the frames before `head` are the row's first thread's.  A
// whole quad is one 16-byte store; its source quad is one 16-byte load where that is aligned too (the same for a whole row), else four
// loads.  Nothing is read or written outside [0, n) of the row.
__global__ __launch_bounds__( 256 ) void k_reverse( const float * __restrict__ in, float * __restrict__ out, int64_t n, int64_t blocks_per_row )
	{
	const int64_t c = int64_t( blockIdx.x ) / blocks_per_row;
	const int64_t q = ( int64_t( blockIdx.x ) - c * blocks_per_row ) * 256 + threadIdx.x;
	const float * src = in + c * n;
	float * dst = out + c * n;
	const int64_t head = std::min<int64_t>( n, int64_t( ( 4 - ( ( reinterpret_cast<uintptr_t>( dst ) >> 2 ) & 3 ) ) & 3 ) );
	if( q == 0 ) for( int64_t f = 0; f < head; ++f ) dst[f] = src[n - 1 - f];
	const int64_t f = head + 4 * q;
	if( f >= n ) return;
	if( f + 4 <= n )
		{
		const float * s = src + ( n - 4 - f );                       // the source quad, ascending: frames n - 4 - f ... n - 1 - f
		float4 v;
		if( ( reinterpret_cast<uintptr_t>( s ) & 15 ) == 0 ) v = *reinterpret_cast<const float4*>( s );
		else v = make_float4( s[0], s[1], s[2], s[3] );
		*reinterpret_cast<float4*>( dst + f ) = make_float4( v.w, v.z, v.y, v.x );
		}
	else
		for( int64_t g = f; g < n; ++g ) dst[g] = src[n - 1 - g];
	}

// ---- launchers --------------------------------------------------------------------------------------------------------------------
int loud_check( const void * audio, int64_t ch, int64_t n, LoudLayout * l )
	{
	FLANHIP_REQUIRE( audio, FLANHIP_ERR_INVALID_ARG, "null buffer" );
	FLANHIP_REQUIRE( ch > 0 && n > 0, FLANHIP_ERR_INVALID_ARG, "non-positive size" );
	FLANHIP_REQUIRE( n <= INT32_MAX, FLANHIP_ERR_INVALID_ARG, "more frames than a Frame counts" );
	FLANHIP_REQUIRE( loud_layout( ch, n, l ), FLANHIP_ERR_INVALID_ARG, "shape out of range" );
	return FLANHIP_OK;
	}

// what the kernels compare against: any gap below -1 acts as -1 and any above INT_MAX as INT_MAX
int64_t loud_gap( int64_t gap ) { return std::clamp<int64_t>( gap, -1, INT32_MAX ); }

int launch_loud_summary( const float * d_audio, int64_t ch, int64_t n, float level, int64_t gap, const LoudLayout & l, int64_t * d_summary, void * d_ws, hipStream_t s )
	{
	LoudMap * tot = ws_at<LoudMap>( d_ws, l.tot ), * carry = ws_at<LoudMap>( d_ws, l.carry );
	uint64_t * masks = ws_at<uint64_t>( d_ws, l.masks );
	auto go = [&]( auto kernel, int64_t blocks, int threads, auto... args ) { return launch_kernel( "launch_loud_summary", kernel, blocks, threads, 0, s, args... ); };
	const bool vec = l.run % 4 == 0 && n % 4 == 0 && aligned16( d_audio );
	if( int rc = scan_pair( vec, [&]( auto V ) { return go( k_loud_sum<V.value>, l.blocks, SCAN_THREADS, d_audio, ch, n, level, loud_gap( gap ), l.run, tot, masks ); } ) ) return rc;
	if( int rc = go( k_scan_carry<LoudMap, LoudMap>, 1, SCAN_THREADS, tot, l.blocks, carry ) ) return rc;
	return go( k_loud_close, 1, 64, tot, carry, l.blocks, d_summary );
	}

int launch_loud_chunks( int64_t n, int64_t gap, const LoudLayout & l, int32_t * d_chunks, int64_t count, void * d_ws, hipStream_t s )
	{
	return launch_kernel( "launch_loud_chunks", k_loud_chunks, l.blocks, SCAN_THREADS, 0, s, ws_at<const uint64_t>( d_ws, l.masks ), ws_at<const LoudMap>( d_ws, l.carry ),
		n, loud_gap( gap ), l.run, d_chunks, count );
	}

int reverse_check( const void * in, int64_t ch, int64_t n, const void * out )
	{
	FLANHIP_REQUIRE( in && out, FLANHIP_ERR_INVALID_ARG, "null buffer" );
	FLANHIP_REQUIRE( ch > 0 && n > 0, FLANHIP_ERR_INVALID_ARG, "non-positive size" );
	FLANHIP_REQUIRE( n <= INT32_MAX && ch <= LOUD_MAX_CHANNELS, FLANHIP_ERR_INVALID_ARG, "shape out of range" );
	const uintptr_t a = reinterpret_cast<uintptr_t>( in ), b = reinterpret_cast<uintptr_t>( out ), bytes = uintptr_t( sizeof( float ) ) * uintptr_t( ch ) * uintptr_t( n );
	FLANHIP_REQUIRE( a + bytes <= b || b + bytes <= a, FLANHIP_ERR_INVALID_ARG, "the output overlaps the input" );
	return FLANHIP_OK;
	}

int launch_reverse( const float * d_in, int64_t ch, int64_t n, float * d_out, hipStream_t s )
	{
	const int64_t quads = ( n + 3 ) / 4 + 1;                          // a head of up to 3 frames may push one quad more
	const int64_t blocks_per_row = ( quads + 255 ) / 256;
	return launch_kernel( "launch_reverse", k_reverse, blocks_per_row * ch, 256, 0, s, d_in, d_out, n, blocks_per_row );
	}

// a time as a Frame (time_to_frame truncated, AudioBuffer.cpp:406-409): false for what no int holds
bool frame_of( float t, float sample_rate, int32_t * frame )
	{
	const float f = t * sample_rate;
	if( !( f > -2147483648.0f && f < 2147483648.0f ) ) return false;
	*frame = int32_t( f );
	return true;
	}
float time_of( int64_t frame, float sample_rate ) { return float( frame ) / sample_rate; }      // frame_to_time( fFrame( frame ) )

} // namespace

} // namespace flanhip

using namespace flanhip;

extern "C" {

size_t flanhip_loud_workspace_bytes( int64_t num_channels, int64_t num_frames )
	{
	LoudLayout l;
	if( !loud_layout( num_channels, num_frames, &l ) ) return 0;
	return l.total;
	}

void flanhip_loud_debug_run( int frames )
	{
	t_loud_run = frames > 0 ? frames : 0;
	}

int64_t flanhip_loud_run_frames( void ) { return scan_run( t_loud_run ); }
int64_t flanhip_loud_block_frames( void ) { return int64_t( scan_run( t_loud_run ) ) * SCAN_THREADS; }
int64_t flanhip_loud_carry_pass_blocks( void ) { return SCAN_THREADS; }

int flanhip_loud_summary_dev( const float * d_audio, int64_t num_channels, int64_t num_frames, float level, int64_t gap_frames, int64_t * d_summary,
	void * d_workspace, void * stream )
	{
	LoudLayout l;
	if( int rc = loud_check( d_audio, num_channels, num_frames, &l ) ) return rc;
	FLANHIP_REQUIRE( d_summary, FLANHIP_ERR_INVALID_ARG, "null buffer" );
	FLANHIP_REQUIRE( d_workspace, FLANHIP_ERR_INVALID_ARG, "null workspace" );
	if( int rc = require_device() ) return rc;
	return launch_loud_summary( d_audio, num_channels, num_frames, level, gap_frames, l, d_summary, d_workspace, (hipStream_t) stream );
	}

int flanhip_loud_chunks_dev( int64_t num_channels, int64_t num_frames, int64_t gap_frames, int64_t count, int32_t * d_chunks, int64_t capacity,
	void * d_workspace, void * stream )
	{
	LoudLayout l;
	FLANHIP_REQUIRE( num_channels > 0 && num_frames > 0, FLANHIP_ERR_INVALID_ARG, "non-positive size" );
	FLANHIP_REQUIRE( num_frames <= INT32_MAX, FLANHIP_ERR_INVALID_ARG, "more frames than a Frame counts" );
	FLANHIP_REQUIRE( loud_layout( num_channels, num_frames, &l ), FLANHIP_ERR_INVALID_ARG, "shape out of range" );
	FLANHIP_REQUIRE( count >= 0 && count <= num_frames, FLANHIP_ERR_INVALID_ARG, "a chunk count the frames cannot hold" );
	FLANHIP_REQUIRE( capacity >= count, FLANHIP_ERR_INVALID_ARG, "the chunk table is smaller than the count" );
	FLANHIP_REQUIRE( d_chunks || capacity == 0, FLANHIP_ERR_INVALID_ARG, "null buffer" );
	FLANHIP_REQUIRE( d_workspace, FLANHIP_ERR_INVALID_ARG, "null workspace" );
	if( int rc = require_device() ) return rc;
	if( count == 0 ) return FLANHIP_OK;
	return launch_loud_chunks( num_frames, gap_frames, l, d_chunks, count, d_workspace, (hipStream_t) stream );
	}

int flanhip_loud_chunks( const float * audio, int64_t num_channels, int64_t num_frames, float level, int64_t gap_frames, int32_t * chunks, int64_t capacity,
	int64_t * summary, volatile int * cancel )
	{
	LoudLayout l;
	if( int rc = loud_check( audio, num_channels, num_frames, &l ) ) return rc;
	FLANHIP_REQUIRE( summary, FLANHIP_ERR_INVALID_ARG, "null buffer" );
	FLANHIP_REQUIRE( capacity >= 0 && ( chunks || capacity == 0 ), FLANHIP_ERR_INVALID_ARG, "null buffer" );
	if( int rc = require_device() ) return rc;
	if( cancelled( cancel ) ) return FLANHIP_ERR_CANCELLED;
	HostCall call( cancel );
	const float * d_audio = nullptr;
	int64_t * d_summary = nullptr;
	void * d_ws = nullptr;
	if( int rc = call.in( audio, sizeof( float ) * size_t( num_channels ) * size_t( num_frames ), &d_audio ) ) return rc;
	if( int rc = call.out( summary, sizeof( int64_t ) * 4, &d_summary ) ) return rc;
	if( int rc = call.scratch( l.total, &d_ws ) ) return rc;
	if( int rc = call.ready() ) return rc;
	if( int rc = launch_loud_summary( d_audio, num_channels, num_frames, level, gap_frames, l, d_summary, d_ws, nullptr ) ) return rc;
	if( int rc = call.finish() ) return rc;                             // the read-back: the count sizes the table
	const int64_t count = summary[0];
	if( capacity == 0 || count == 0 ) return FLANHIP_OK;                // the summary alone
	FLANHIP_REQUIRE( capacity >= count, FLANHIP_ERR_INVALID_ARG, "the chunk table is smaller than the count" );
	HostCall table( cancel );
	int32_t * d_chunks = nullptr;
	if( int rc = table.out( chunks, sizeof( int32_t ) * 2 * size_t( count ), &d_chunks ) ) return rc;
	if( int rc = launch_loud_chunks( num_frames, gap_frames, l, d_chunks, count, d_ws, nullptr ) ) return rc;
	return table.finish();
	}

int flanhip_audio_reverse_dev( const float * d_audio, int64_t num_channels, int64_t num_frames, float * d_out, void * stream )
	{
	if( int rc = reverse_check( d_audio, num_channels, num_frames, d_out ) ) return rc;
	if( int rc = require_device() ) return rc;
	return launch_reverse( d_audio, num_channels, num_frames, d_out, (hipStream_t) stream );
	}

int flanhip_audio_reverse( const float * audio, int64_t num_channels, int64_t num_frames, float * out, volatile int * cancel )
	{
	if( int rc = reverse_check( audio, num_channels, num_frames, out ) ) return rc;
	if( int rc = require_device() ) return rc;
	if( cancelled( cancel ) ) return FLANHIP_ERR_CANCELLED;
	const size_t bytes = sizeof( float ) * size_t( num_channels ) * size_t( num_frames );
	HostCall call( cancel );
	const float * d_in = nullptr;
	float * d_out = nullptr;
	if( int rc = call.in( audio, bytes, &d_in ) ) return rc;
	if( int rc = call.out( out, bytes, &d_out ) ) return rc;
	if( int rc = call.ready() ) return rc;
	if( int rc = launch_reverse( d_in, num_channels, num_frames, d_out, nullptr ) ) return rc;
	return call.finish();
	}

// ---- host arithmetic ----------------------------------------------------------------------------------------------------------------
int flanhip_loud_chunks_fades( int64_t num_frames, float sample_rate, const int32_t * chunks, int64_t count, float fade_in_time, int join,
	flanhip_grain_event * events, float * offsets )
	{
	FLANHIP_REQUIRE( chunks && events, FLANHIP_ERR_INVALID_ARG, "null buffer" );
	FLANHIP_REQUIRE( num_frames > 0 && count > 0, FLANHIP_ERR_INVALID_ARG, "non-positive size" );
	FLANHIP_REQUIRE( num_frames <= INT32_MAX, FLANHIP_ERR_INVALID_ARG, "more frames than a Frame counts" );
	FLANHIP_REQUIRE( sample_rate > 0, FLANHIP_ERR_INVALID_ARG, "sample_rate <= 0" );
	FLANHIP_REQUIRE( flanhip_grains_workspace_bytes( count, 1 ) != 0, FLANHIP_ERR_INVALID_ARG, "a table longer than the mix takes" );
	for( int64_t i = 0; i < count; ++i )
		FLANHIP_REQUIRE( chunks[2 * i] >= 0 && chunks[2 * i] <= chunks[2 * i + 1] && chunks[2 * i + 1] <= num_frames, FLANHIP_ERR_INVALID_ARG, "a chunk outside the frames" );
	std::vector<float> fade_ins( size_t( count ) + 1, fade_in_time );                // :52
	for( int64_t i = 0; i < count; ++i )                                             // :55-64: iteration i reads what i - 1 left in fade_ins[i]
		{
		int32_t fade_frames_i;
		FLANHIP_REQUIRE( frame_of( fade_ins[size_t( i )], sample_rate, &fade_frames_i ), FLANHIP_ERR_INVALID_ARG, "a fade time no frame holds" );
		const int64_t c0 = chunks[2 * i], c1 = chunks[2 * i + 1];
		fade_ins[size_t( i )] = time_of( c0 - fade_frames_i < 0 ? c0 : fade_frames_i, sample_rate );
		fade_ins[size_t( i ) + 1] = time_of( c1 + fade_frames_i >= num_frames ? num_frames - c1 : fade_frames_i, sample_rate );
		}
	std::vector<int32_t> start( static_cast<size_t>( count ) ), end( start.size() ), left( start.size() ), right( start.size() );
	for( int64_t i = 0; i < count; ++i )                                             // :70-79
		{
		int32_t l, r;
		FLANHIP_REQUIRE( frame_of( fade_ins[size_t( i )], sample_rate, &l ) && frame_of( fade_ins[size_t( i ) + 1], sample_rate, &r ), FLANHIP_ERR_INVALID_ARG,
			"a fade time no frame holds" );
		const int64_t s = int64_t( chunks[2 * i] ) - l, e = int64_t( chunks[2 * i + 1] ) + r;
		FLANHIP_REQUIRE( s >= INT32_MIN && e <= INT32_MAX, FLANHIP_ERR_INVALID_ARG, "a fade time no frame holds" );
		start[size_t( i )] = int32_t( s ); end[size_t( i )] = int32_t( e ); left[size_t( i )] = l; right[size_t( i )] = r;
		}
	if( int rc = flanhip_grains_cut_frames( num_frames, count, start.data(), end.data(), left.data(), right.data(), events ) ) return rc;
	if( offsets ) for( int64_t i = 0; i <= count; ++i ) offsets[i] = -2 * fade_ins[size_t( i )];      // :82-83
	if( !join ) return FLANHIP_OK;
	float start_time = 0;                                                            // AudioCombination.cpp:212-218, then :127-129
	for( int64_t i = 0; i < count; ++i )
		{
		int32_t o;
		FLANHIP_REQUIRE( frame_of( start_time, sample_rate, &o ), FLANHIP_ERR_INVALID_ARG, "a start time no frame holds" );
		events[i].o = o;
		start_time = start_time + float( events[i].n ) / sample_rate + -2 * fade_ins[size_t( i ) + 1];
		}
	return FLANHIP_OK;
	}

int flanhip_edge_silence_cut( int64_t num_frames, float sample_rate, int64_t first_noisy, int64_t last_noisy, float fade_time, int32_t * out4 )
	{
	FLANHIP_REQUIRE( out4, FLANHIP_ERR_INVALID_ARG, "null buffer" );
	FLANHIP_REQUIRE( num_frames > 0, FLANHIP_ERR_INVALID_ARG, "non-positive size" );
	FLANHIP_REQUIRE( num_frames <= INT32_MAX, FLANHIP_ERR_INVALID_ARG, "more frames than a Frame counts" );
	FLANHIP_REQUIRE( sample_rate > 0, FLANHIP_ERR_INVALID_ARG, "sample_rate <= 0" );
	FLANHIP_REQUIRE( ( first_noisy == -1 && last_noisy == -1 ) || ( first_noisy >= 0 && first_noisy <= last_noisy && last_noisy < num_frames ), FLANHIP_ERR_INVALID_ARG,
		"noisy frames outside the frames" );
	int32_t fade_frames;
	FLANHIP_REQUIRE( frame_of( fade_time, sample_rate, &fade_frames ), FLANHIP_ERR_INVALID_ARG, "a fade time no frame holds" );
	// :129-147: nothing noisy walks start_frame up to num_frames and end_frame down to 0
	const int64_t start_frame = first_noisy < 0 ? num_frames : first_noisy, end_frame = last_noisy < 0 ? 0 : last_noisy + 1;
	const int64_t start_fade = start_frame - fade_frames < 0 ? start_frame : fade_frames;                     // :150
	const int64_t end_fade = end_frame + fade_frames >= num_frames ? num_frames - end_frame : fade_frames;   // :151
	const int64_t s = start_frame - fade_frames, e = end_frame + fade_frames;
	FLANHIP_REQUIRE( s >= INT32_MIN && e <= INT32_MAX, FLANHIP_ERR_INVALID_ARG, "a fade time no frame holds" );
	out4[0] = int32_t( s ); out4[1] = int32_t( e ); out4[2] = int32_t( start_fade ); out4[3] = int32_t( end_fade );      // :152
	return FLANHIP_OK;
	}

int flanhip_split_frames( int64_t num_frames, float sample_rate, const float * times, int64_t count, int32_t * frames, int64_t capacity, int64_t * out_count )
	{
	FLANHIP_REQUIRE( out_count, FLANHIP_ERR_INVALID_ARG, "null buffer" );
	FLANHIP_REQUIRE( num_frames > 0 && count >= 0, FLANHIP_ERR_INVALID_ARG, "non-positive size" );
	FLANHIP_REQUIRE( num_frames <= INT32_MAX, FLANHIP_ERR_INVALID_ARG, "more frames than a Frame counts" );
	FLANHIP_REQUIRE( sample_rate > 0, FLANHIP_ERR_INVALID_ARG, "sample_rate <= 0" );
	FLANHIP_REQUIRE( times || count == 0, FLANHIP_ERR_INVALID_ARG, "null buffer" );
	FLANHIP_REQUIRE( capacity >= 0 && ( frames || capacity == 0 ), FLANHIP_ERR_INVALID_ARG, "null buffer" );
	FLANHIP_REQUIRE( flanhip_grains_workspace_bytes( count + 1, 1 ) != 0, FLANHIP_ERR_INVALID_ARG, "a table longer than the mix takes" );
	for( int64_t i = 0; i < count; ++i ) FLANHIP_REQUIRE( times[i] == times[i], FLANHIP_ERR_INVALID_ARG, "a split time that is not a number" );
	std::vector<float> sorted( times, times + count );
	std::sort( sorted.begin(), sorted.end() );                                       // :418
	std::vector<int32_t> split = { 0 };                                              // :420-429
	for( float t : sorted )
		{
		const float f = t * sample_rate;
		if( !( f < 2147483648.0f ) ) break;                                          // beyond every Frame: beyond num_frames
		if( !( f > -2147483648.0f ) ) continue;
		const int32_t frame = int32_t( f );
		if( frame <= 0 ) continue;
		if( num_frames <= frame ) break;
		split.push_back( frame );
		}
	split.push_back( int32_t( num_frames ) );
	*out_count = int64_t( split.size() );
	if( capacity == 0 ) return FLANHIP_OK;                                           // the count alone
	FLANHIP_REQUIRE( capacity >= int64_t( split.size() ), FLANHIP_ERR_INVALID_ARG, "the frame buffer is too small" );
	std::copy( split.begin(), split.end(), frames );
	return FLANHIP_OK;
	}

int flanhip_rearrange_order( int64_t count, uint64_t seed, int32_t * order )
	{
	FLANHIP_REQUIRE( order, FLANHIP_ERR_INVALID_ARG, "null buffer" );
	FLANHIP_REQUIRE( count > 0, FLANHIP_ERR_INVALID_ARG, "non-positive size" );
	FLANHIP_REQUIRE( flanhip_grains_workspace_bytes( count, 1 ) != 0, FLANHIP_ERR_INVALID_ARG, "a table longer than the mix takes" );
	for( int64_t i = 0; i < count; ++i ) order[i] = int32_t( i );
	std::mt19937 g( static_cast<uint32_t>( seed ) );
	for( int64_t i = count - 1; i > 0; --i ) std::swap( order[i], order[int64_t( g() % uint32_t( i + 1 ) )] );
	return FLANHIP_OK;
	}

int64_t flanhip_random_chunks_frames( float sample_rate, float length )
	{
	if( !( sample_rate > 0 ) ) return -1;
	const float end = length * sample_rate;                                          // time_to_frame( length ), a float (:496)
	if( !( end > 0 ) || !( end < 2147483648.0f ) ) return -1;
	int64_t frames = int64_t( end );
	if( float( frames ) < end ) ++frames;                                            // the loop's condition compares Frame with fFrame
	return frames;
	}

int flanhip_random_chunks_plan( int64_t num_frames, float sample_rate, float length, const float * chunk_length, float chunk_length_scalar, const float * fade,
	float fade_scalar, uint64_t seed, flanhip_grain_event * events, int32_t * chunk_starts, float * offsets, int64_t capacity, int64_t * out_count )
	{
	FLANHIP_REQUIRE( out_count, FLANHIP_ERR_INVALID_ARG, "null buffer" );
	FLANHIP_REQUIRE( num_frames > 0, FLANHIP_ERR_INVALID_ARG, "non-positive size" );
	FLANHIP_REQUIRE( num_frames <= INT32_MAX, FLANHIP_ERR_INVALID_ARG, "more frames than a Frame counts" );
	FLANHIP_REQUIRE( sample_rate > 0, FLANHIP_ERR_INVALID_ARG, "sample_rate <= 0" );
	const int64_t loop_frames = flanhip_random_chunks_frames( sample_rate, length );
	FLANHIP_REQUIRE( loop_frames > 0, FLANHIP_ERR_INVALID_ARG, "non-positive size" );
	FLANHIP_REQUIRE( capacity >= 0 && ( capacity == 0 || ( events && chunk_starts && offsets ) ), FLANHIP_ERR_INVALID_ARG, "null buffer" );
	const int32_t end_frame = int32_t( length * sample_rate );                        // :509
	const float lowest = time_of( 32, sample_rate ), longest = time_of( num_frames, sample_rate );       // :505
	std::vector<int32_t> starts;                                                     // :494-509
	double accumulator = 1;
	for( int64_t f = 0; f < loop_frames; ++f )
		{
		if( accumulator >= 1 )
			{
			starts.push_back( int32_t( f ) );
			accumulator = std::fmod( accumulator, 1.0 );
			}
		const float wanted = chunk_length ? chunk_length[f] : chunk_length_scalar;
		const double seconds_per_chunk = std::clamp( wanted, lowest, longest );      // std::clamp in fp32, then widened
		accumulator += 1.0 / seconds_per_chunk / sample_rate;
		}
	starts.push_back( end_frame );
	const int64_t count = int64_t( starts.size() ) - 1;
	FLANHIP_REQUIRE( flanhip_grains_workspace_bytes( count, 1 ) != 0, FLANHIP_ERR_INVALID_ARG, "a table longer than the mix takes" );
	*out_count = count;
	if( capacity == 0 ) return FLANHIP_OK;                                           // the count alone
	FLANHIP_REQUIRE( capacity >= count, FLANHIP_ERR_INVALID_ARG, "the event buffer is too small" );
	std::vector<float> fades( starts.size() );                                       // :517-519: fade at the chunk's start time
	for( size_t i = 0; i < starts.size(); ++i ) fades[i] = fade ? fade[std::min<int64_t>( starts[i], loop_frames )] : fade_scalar;
	std::mt19937 rng( static_cast<uint32_t>( seed ) );
	std::vector<int32_t> s( static_cast<size_t>( count ) ), e( s.size() ), sf( s.size() ), ef( s.size() );
	for( int64_t i = 0; i < count; ++i )                                             // :525-533
		{
		int32_t both, left, right;
		FLANHIP_REQUIRE( frame_of( ( fades[size_t( i )] + fades[size_t( i ) + 1] ) / 2, sample_rate, &both ) && frame_of( fades[size_t( i )], sample_rate, &left )
			&& frame_of( fades[size_t( i ) + 1], sample_rate, &right ), FLANHIP_ERR_INVALID_ARG, "a fade time no frame holds" );
		const int64_t desired = int64_t( starts[size_t( i ) + 1] ) - starts[size_t( i )] + both;
		FLANHIP_REQUIRE( desired <= INT32_MAX && desired >= INT32_MIN, FLANHIP_ERR_INVALID_ARG, "a fade time no frame holds" );
		const int64_t start_frame = desired >= num_frames ? 0 : int64_t( rng() % uint32_t( num_frames - desired ) );
		FLANHIP_REQUIRE( start_frame + desired <= INT32_MAX, FLANHIP_ERR_INVALID_ARG, "a fade time no frame holds" );
		s[size_t( i )] = int32_t( start_frame ); e[size_t( i )] = int32_t( start_frame + desired ); sf[size_t( i )] = left; ef[size_t( i )] = right;
		chunk_starts[i] = starts[size_t( i )];
		}
	if( int rc = flanhip_grains_cut_frames( num_frames, count, s.data(), e.data(), sf.data(), ef.data(), events ) ) return rc;
	for( int64_t i = 0; i <= count; ++i ) offsets[i] = -fades[size_t( i )];          // :542-544
	float start_time = 0;                                                            // AudioCombination.cpp:212-218, then :127-129
	for( int64_t i = 0; i < count; ++i )
		{
		int32_t o;
		FLANHIP_REQUIRE( frame_of( start_time, sample_rate, &o ), FLANHIP_ERR_INVALID_ARG, "a start time no frame holds" );
		events[i].o = o;
		start_time = start_time + float( events[i].n ) / sample_rate + offsets[i + 1];
		}
	return FLANHIP_OK;
	}

} // extern "C"
