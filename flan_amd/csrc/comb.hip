// comb.hip -- Audio::filter_comb (Audio/AudioFilter.cpp:988-1043): the feedback comb with a per-frame delay.  DESIGN.md section 4.18.
//
// The reference runs one sequential loop per channel:
//   u[n] = x[n] + ( k f ) u[p(n)],      y[n] = a u[n] + ( ( 1 - a ) f ) u[p(n)],      p(n) = trunc( float( n ) - ( 1 / ( 2 w ) ) sr )
// with the cutoff w, the feedback k and the mix a sampled per frame, f = +-1, and u[p] read as 0 where p is outside the signal or is the
// frame itself.  The delay n - p(n) changes every frame, so this is no scan of a fixed-size state (run_scan.h does not fit): every frame
// hangs on at most ONE earlier frame, the frames are a forest, and u is a linear recurrence along its paths.  The parallel form is pointer
// jumping.  With the invariant u[n] = X[n] + C[n] u[P[n]] (P = -1: u[n] = X[n]), from X = x, C = k f, P = p, a round does for every frame
//   q = P[n] >= 0:   X[n] += C[n] X[q],   C[n] *= C[q],   P[n] = P[q]
// which doubles the distance every live link spans: after ceil( log2 n ) rounds no link is left and X = u.  Here:
//   k_comb_link      one thread per frame, once for all channels: p[n] and c[n] = k f, the reference's fp32 arithmetic, c widened to fp64
//   k_comb_jump      one round, all in fp64.  It reads one buffer and writes the other: a frame's parent may be in any other block, so a round in
//                    place would race.  The first round reads the fp32 input itself, widened as it is read.  A finished frame is copied.
//   k_comb_local     (a scalar cutoff) the first rounds of every tile of 2048 frames in LDS, in one launch: the same operations on the same
//                    values as that many launches of k_comb_jump, so no output bit depends on it; a tile checks that its halo holds
//                    the ancestors it needs, and if one does not, every round runs globally as if this launch had not been
//   k_comb_out       u rounded to fp32 once, the link computed again from the cutoff, the output line in the reference's fp32 operations
// The host launches every round it may need and reads nothing back.  A round leaves a word for the next one that says whether any live
// link is left, and a round that finds its word 0 returns at once; k_comb_out counts the words that are set and so knows which buffer holds
// u.  Launch boundaries order everything: no block waits for another, no flags inside a launch, no atomics (the word is a plain store of
// 1, by whoever has a live link).  Every frame's value comes from a fixed sequence of operations -- which rounds touch it depends on the
// links alone --, so two calls agree bit for bit and a channel's output does not depend on the channels filtered with it or on the grid.
#include "flanhip_internal.h"

namespace flanhip {

namespace {

constexpr int COMB_THREADS = 256;
constexpr int COMB_GROUP = 8;                                  // channels one thread carries a frame for
constexpr int COMB_WORDS = 64;                                 // the words at the head of the workspace: [r] != 0, r < 32: round r has live links to follow
constexpr int COMB_WORD_FAIL = 32;                             // != 0: a tile of k_comb_local could not bring its frames to the level asked for
constexpr int COMB_WORD_DONE = 33;                             // left by k_comb_out: the rounds X went through
constexpr int COMB_SPAN = 2048;                                // the frames of a tile of k_comb_local, halo included: 40 bytes of LDS each
constexpr int COMB_LOCAL_THREADS = 1024;                       // of a block of k_comb_local: two blocks a CU by their LDS, 32 wavefronts
constexpr int COMB_MAX_LOCAL = 9;                              // the rounds a tile runs at most: a halo of 511 links
thread_local int t_comb_local = 0;                             // flanhip_filter_comb_debug_local: 0 the library's choice, < 0 off, > 0 the rounds forced
constexpr int64_t COMB_MAX_FRAMES = ( int64_t( 1 ) << 31 ) - 1;      // the links are int32
constexpr int64_t COMB_MAX_CHANNELS = 1 << 20;

struct CombLayout
	{
	int64_t blocks = 0, groups = 0;       // blocks of COMB_THREADS frames; groups of COMB_GROUP channels
	size_t X = 0, C = 0, P = 0, total = 0;
	};

// the workspace: COMB_WORDS words, the planes X[2][ch][n] (fp64), the rows C[2][n] (fp64), the rows P[2][n] (int32)
bool comb_layout( int64_t ch, int64_t n, CombLayout * l )
	{
	if( ch <= 0 || n <= 0 || ch > COMB_MAX_CHANNELS || n > COMB_MAX_FRAMES ) return false;
	l->blocks = ( n + COMB_THREADS - 1 ) / COMB_THREADS;
	l->groups = ( ch + COMB_GROUP - 1 ) / COMB_GROUP;
	if( l->blocks > COMB_MAX_FRAMES / l->groups ) return false;
	const size_t N = size_t( n ), plane = sizeof( double ) * N;
	l->X = sizeof( int ) * COMB_WORDS;
	l->C = l->X + 2 * plane * size_t( ch );
	l->P = l->C + 2 * plane;
	l->total = l->P + 2 * sizeof( int ) * N;
	return true;
	}

// :1009 std::clamp( c, 1.0f, sr / 2.0f ): two comparisons, a NaN stays
__host__ __device__ __forceinline__ float comb_clamp( float cutoff, float nyquist ) { return cutoff < 1.0f ? 1.0f : nyquist < cutoff ? nyquist : cutoff; }
// :1031 delay = 1.0f / ( 2.0f * w ); AudioBuffer.cpp:406-409 time_to_frame( delay ) = delay * sr
__host__ __device__ __forceinline__ float comb_delay_frames( float cutoff, float sr )
	{
	const float w = comb_clamp( cutoff, sr / 2.0f );
	const float delay = 1.0f / ( 2.0f * w );
	return delay * sr;
	}
// :1032 Frame( float( frame ) - d ), truncated toward zero, through safe_u_access (:1016-1020): the frame u is read at, or -1 where it reads 0.
// t in ( -1, 0 ) truncates to 0.  p == n (n = 0 with d < 1) reads u[0] before it is written, which is 0.  A NaN t (a NaN cutoff) and a t
// of 2^31 or more are an undefined cast, INT_MIN on x86, which safe_u_access turns into 0: no link
__host__ __device__ __forceinline__ int comb_link( int64_t n, float d )
	{
	const float t = float( n ) - d;
	if( !( t > -1.0f && t < 2147483648.0f ) ) return -1;
	const int64_t p = int64_t( t );
	return p < n ? int( p ) : -1;
	}

// ---- kernels ----------------------------------------------------------------------------------------------------------------------
// one frame per thread, once for all channels: the link and c = k * f (:1035).  words[0]: some frame has a link
__global__ __launch_bounds__( COMB_THREADS ) void k_comb_link( const float * __restrict__ cutoff, float cutoff_c, const float * __restrict__ feedback,
	float feedback_c, float sign, float sr, int64_t n, int * __restrict__ P, double * __restrict__ C, int * words )
	{
	const int64_t f = int64_t( blockIdx.x ) * COMB_THREADS + threadIdx.x;
	int p = -1;
	if( f < n )
		{
		p = comb_link( f, comb_delay_frames( cutoff ? cutoff[f] : cutoff_c, sr ) );
		const float c = ( feedback ? feedback[f] : feedback_c ) * sign;
		P[f] = p;
		C[f] = double( c );
		}
	if( __ballot( p >= 0 ) && ( threadIdx.x & 63 ) == 0 ) words[0] = 1;
	}

// One round from buffer `from` to the other one.  A thread carries frame f for the channels of its group and updates the pair ( P, C ) once
// (group 0 writes it).  FIRST: the round that reads the fp32 input instead of a plane X
template<bool FIRST>
__global__ __launch_bounds__( COMB_THREADS ) void k_comb_jump( const float * __restrict__ audio, int64_t ch, int64_t n, int64_t blocks, int round, int local,
	const double * __restrict__ X_from, double * __restrict__ X_to, const double * __restrict__ C_from, double * __restrict__ C_to,
	const int * __restrict__ P_from, int * __restrict__ P_to, int * words )
	{
	if( round < local && words[COMB_WORD_FAIL] == 0 ) return;          // k_comb_local ran this round in LDS
	if( words[round] == 0 ) return;                                    // the round before left no live link (or there never was one)
	const int64_t group = int64_t( blockIdx.x ) / blocks;
	const int64_t f = ( int64_t( blockIdx.x ) - group * blocks ) * COMB_THREADS + threadIdx.x;
	int p_new = -1;
	if( f < n )
		{
		const int q = P_from[f];
		const double c = C_from[f];
		const int64_t c0 = group * COMB_GROUP, c1 = c0 + COMB_GROUP < ch ? c0 + COMB_GROUP : ch;
		for( int64_t channel = c0; channel < c1; ++channel )
			{
			const int64_t row = channel * n;
			double x, xq = 0.0;
			if constexpr( FIRST ) { x = double( audio[row + f] ); if( q >= 0 ) xq = double( audio[row + q] ); }
			else { x = X_from[row + f]; if( q >= 0 ) xq = X_from[row + q]; }
			X_to[row + f] = q >= 0 ? x + c * xq : x;
			}
		double c_new = c;
		if( q >= 0 ) { c_new = c * C_from[q]; p_new = P_from[q]; }
		if( group == 0 ) { C_to[f] = c_new; P_to[f] = p_new; }
		}
	if( group == 0 && __ballot( p_new >= 0 ) && ( threadIdx.x & 63 ) == 0 ) words[round + 1] = 1;
	}

// The first `rounds` rounds of a tile in LDS, in one pass.  A block takes one channel's tile: `own` frames and, before them, a halo of
// `halo` frames that it computes and does not write.  Rounds are synchronous -- round r of a frame needs what round r - 1 left of its
// parent --, so a frame goes through a round only if its parent is in the tile and went through the round before; otherwise its link
// is marked -2 and so is, a round later, every frame that reads it.  A tile whose OWN frames all went through all the rounds writes
// exactly what `rounds` launches of k_comb_jump would have written of them, into the buffers the last of these would have written
// (`rounds` is odd: buffer 1, which the global round 0 overwrites, never the link rows in buffer 0); a tile that did not raises
// words[COMB_WORD_FAIL], and then every global round runs as if this kernel had not.  Block 0's channel writes the pair ( P, C )
__global__ __launch_bounds__( COMB_LOCAL_THREADS ) void k_comb_local( const float * __restrict__ audio, int64_t n, int64_t tiles, int rounds, int own, int halo,
	const int * __restrict__ P0, const double * __restrict__ C0, double * __restrict__ X_to, double * __restrict__ C_to, int * __restrict__ P_to, int * words )
	{
	extern __shared__ double s_comb[];
	if( words[0] == 0 ) return;                                        // no frame has a link
	// the two buffers of X, of C and of P, one after the other
	auto sX = [&]( int buffer ) { return s_comb + buffer * COMB_SPAN; };
	auto sC = [&]( int buffer ) { return s_comb + ( 2 + buffer ) * COMB_SPAN; };
	auto sP = [&]( int buffer ) { return reinterpret_cast<int*>( s_comb + 4 * COMB_SPAN ) + buffer * COMB_SPAN; };
	const int64_t channel = int64_t( blockIdx.x ) / tiles, tile = int64_t( blockIdx.x ) - channel * tiles;
	const int64_t first_own = tile * own, start = first_own > halo ? first_own - halo : 0, end = first_own + own < n ? first_own + own : n;
	const int span = int( end - start ), skip = int( first_own - start );
	const int64_t row = channel * n;
	for( int i = threadIdx.x; i < span; i += COMB_LOCAL_THREADS )
		{
		sX( 0 )[i] = double( audio[row + start + i] );
		sC( 0 )[i] = C0[start + i];
		sP( 0 )[i] = P0[start + i];
		}
	__syncthreads();
	for( int r = 0; r < rounds; ++r )
		{
		const int from = r & 1, to = from ^ 1;
		const double * X_from = sX( from ), * C_from = sC( from );
		const int * P_from = sP( from );
		for( int i = threadIdx.x; i < span; i += COMB_LOCAL_THREADS )
			{
			const int q = P_from[i];
			double x = X_from[i], c = C_from[i];
			int p = q;
			if( q >= 0 )
				{
				const int64_t j = q - start;
				const int pq = j >= 0 ? P_from[j] : -2;
				if( pq == -2 ) p = -2;
				else { x = x + c * X_from[j]; c = c * C_from[j]; p = pq; }
				}
			sX( to )[i] = x; sC( to )[i] = c; sP( to )[i] = p;
			}
		__syncthreads();
		}
	const int last = rounds & 1;
	bool failed = false, live = false;
	for( int i = skip + threadIdx.x; i < span; i += COMB_LOCAL_THREADS )
		{
		const int p = sP( last )[i];
		failed = failed || p == -2;
		live = live || p >= 0;
		X_to[row + start + i] = sX( last )[i];
		if( channel == 0 ) { C_to[start + i] = sC( last )[i]; P_to[start + i] = p; }
		}
	if( __ballot( failed ) && ( threadIdx.x & 63 ) == 0 ) words[COMB_WORD_FAIL] = 1;
	if( channel == 0 && __ballot( live ) && ( threadIdx.x & 63 ) == 0 ) words[rounds] = 1;
	}

// u rounded to fp32 once and the output line (:1038).  The rounds that did work are the words set among the first `rounds`; an even count
// leaves u in plane 0 -- no round at all: in the input itself --, an odd one in plane 1.  out may be the audio: with no round no frame has
// a link and a thread reads the one sample it writes; otherwise the audio is not read
__global__ __launch_bounds__( COMB_THREADS ) void k_comb_out( const float * audio, int64_t ch, int64_t n, int64_t blocks, int rounds, int local, float sr,
	const float * __restrict__ cutoff, float cutoff_c, const float * __restrict__ wet_dry, float wet_dry_c, float sign,
	const double * __restrict__ X0, const double * __restrict__ X1, int * words, float * out )
	{
	// with the tiles' rounds done in LDS (some frame has a link and no tile failed) the global rounds began at round `local`
	const int first = words[0] != 0 && words[COMB_WORD_FAIL] == 0 ? local : 0;
	int done = first;
	for( int r = first; r < rounds; ++r ) done += words[r] != 0;
	if( blockIdx.x == 0 && threadIdx.x == 0 ) words[COMB_WORD_DONE] = done;
	const double * X = done & 1 ? X1 : X0;
	const int64_t group = int64_t( blockIdx.x ) / blocks;
	const int64_t f = ( int64_t( blockIdx.x ) - group * blocks ) * COMB_THREADS + threadIdx.x;
	if( f >= n ) return;
	const int p = comb_link( f, comb_delay_frames( cutoff ? cutoff[f] : cutoff_c, sr ) );
	const float a = wet_dry ? wet_dry[f] : wet_dry_c;
	const float b = ( 1.0f - a ) * sign;
	const int64_t c0 = group * COMB_GROUP, c1 = c0 + COMB_GROUP < ch ? c0 + COMB_GROUP : ch;
	for( int64_t channel = c0; channel < c1; ++channel )
		{
		const int64_t row = channel * n;
		float u, um = 0.0f;
		if( done == 0 ) u = audio[row + f];
		else { u = float( X[row + f] ); if( p >= 0 ) um = float( X[row + p] ); }
		out[row + f] = a * u + b * um;
		}
	}

// ---- launcher ---------------------------------------------------------------------------------------------------------------------
struct CombArgs
	{
	const float * audio; int64_t ch, n; float sr;
	const float * cutoff; float cutoff_c;
	const float * feedback; float feedback_c;
	const float * wet_dry; float wet_dry_c;
	int invert;
	float * out;
	};

// what both forms refuse before any device call
int comb_check( const CombArgs & a, CombLayout * l )
	{
	FLANHIP_REQUIRE( a.audio && a.out, FLANHIP_ERR_INVALID_ARG, "null buffer" );
	FLANHIP_REQUIRE( a.ch > 0 && a.n > 0, FLANHIP_ERR_INVALID_ARG, "non-positive size" );
	FLANHIP_REQUIRE( a.sr > 0.0f, FLANHIP_ERR_INVALID_ARG, "sample rate not positive" );
	FLANHIP_REQUIRE( comb_layout( a.ch, a.n, l ), FLANHIP_ERR_UNSUPPORTED, "shape out of range" );
	return FLANHIP_OK;
	}

// The rounds to launch: ceil( log2 n ) resolve any forest of n frames.  A scalar cutoff gives every link the same d: below 2^24 frames
// float( n ) is exact, a link spans at least D = max( trunc d, 1 ) frames, a path has at most ceil( n / D ) frames, and
// ceil( log2 ceil( n / D ) ) rounds resolve it; one more is launched and finds nothing to do
int comb_rounds( const CombArgs & a )
	{
	const int full = ilog2( a.n );
	if( a.cutoff || a.n > ( int64_t( 1 ) << 24 ) ) return full;
	const float d = comb_delay_frames( a.cutoff_c, a.sr );
	const int64_t D = d >= float( a.n ) ? a.n : d >= 1.0f ? int64_t( d ) : 1;        // a NaN d: 1
	return std::min( full, ilog2( ( a.n + D - 1 ) / D ) + 1 );
	}

// The rounds to run tile-local first (k_comb_local), an odd number or 0, and the halo for them.  A frame needs its 2^k - 1 nearest
// ancestors in the tile.  With a scalar cutoff and float( n ) exact a link spans at most ceil( d ) frames: the halo is sized for that, as
// many rounds as half a tile's span allows, and no tile fails.  With a curve the host does not know the delays, a call with one failing
// tile pays for the launch and gets nothing, and 3 rounds behind half a span gained 1 % where they worked: none.  A
// forced count (the debug hook) runs behind half a span whatever the cutoff
int comb_local_rounds( const CombArgs & a, int rounds, int * halo )
	{
	int k = 0;
	*halo = COMB_SPAN / 2;
	if( t_comb_local < 0 ) return 0;
	if( t_comb_local > 0 ) k = std::min( t_comb_local, COMB_MAX_LOCAL );
	else if( !a.cutoff && a.n <= ( int64_t( 1 ) << 24 ) )
		{
		const float d = comb_delay_frames( a.cutoff_c, a.sr );
		if( !( d <= float( COMB_SPAN / 2 ) ) ) return 0;                  // a NaN d as well: no links
		const int D = int( ceilf( d ) );
		k = 0;
		while( k < COMB_MAX_LOCAL && ( ( int64_t( 2 ) << k ) - 1 ) * D <= COMB_SPAN / 2 ) ++k;
		*halo = ( ( 1 << k ) - 1 ) * D;
		}
	k = std::min( k, rounds );
	return k > 0 && k % 2 == 0 ? k - 1 : k;
	}

// cancel (the host form's flag, or null) is polled between the rounds
int launch_comb( const CombArgs & a, void * d_ws, hipStream_t s, volatile int * cancel = nullptr )
	{
	CombLayout l;
	if( int rc = comb_check( a, &l ) ) return rc;
	FLANHIP_REQUIRE( d_ws, FLANHIP_ERR_INVALID_ARG, "null workspace" );
	if( int rc = require_device() ) return rc;
	auto go = [&]( auto kernel, int64_t blocks, auto... args ) { return launch_kernel( "launch_comb", kernel, blocks, COMB_THREADS, 0, s, args... ); };
	const int64_t ch = a.ch, n = a.n, grid = l.blocks * l.groups;
	const size_t N = size_t( n );
	int * words = ws_at<int>( d_ws, 0 );
	double * X[2] = { ws_at<double>( d_ws, l.X ), ws_at<double>( d_ws, l.X ) + size_t( ch ) * N };
	double * C[2] = { ws_at<double>( d_ws, l.C ), ws_at<double>( d_ws, l.C ) + N };
	int * P[2] = { ws_at<int>( d_ws, l.P ), ws_at<int>( d_ws, l.P ) + N };
	const float sign = a.invert ? -1.0f : 1.0f;                           // :1006
	const int rounds = comb_rounds( a );
	int halo = 0;
	const int local = comb_local_rounds( a, rounds, &halo );
	FLANHIP_CHECK( hipMemsetAsync( words, 0, sizeof( int ) * COMB_WORDS, s ) );
	if( int rc = go( k_comb_link, l.blocks, a.cutoff, a.cutoff_c, a.feedback, a.feedback_c, sign, a.sr, n, P[0], C[0], words ) ) return rc;
	if( local )
		{
		if( cancelled( cancel ) ) return FLANHIP_ERR_CANCELLED;
		const int own = COMB_SPAN - halo;
		const int64_t tiles = ( n + own - 1 ) / own;
		FLANHIP_REQUIRE( tiles <= COMB_MAX_FRAMES / ch, FLANHIP_ERR_UNSUPPORTED, "shape out of range" );
		if( int rc = launch_kernel( "launch_comb", k_comb_local, tiles * ch, COMB_LOCAL_THREADS, COMB_SPAN * ( 4 * sizeof( double ) + 2 * sizeof( int ) ), s,
			a.audio, n, tiles, local, own, halo, (const int*) P[0], (const double*) C[0], X[1], C[1], P[1], words ) ) return rc;
		}
	for( int r = 0; r < rounds; ++r )
		{
		if( cancelled( cancel ) ) return FLANHIP_ERR_CANCELLED;
		const int from = r & 1, to = from ^ 1;
		const int rc = r == 0
			? go( k_comb_jump<true>, grid, a.audio, ch, n, l.blocks, r, local, (const double*) X[from], X[to], (const double*) C[from], C[to], (const int*) P[from], P[to], words )
			: go( k_comb_jump<false>, grid, a.audio, ch, n, l.blocks, r, local, (const double*) X[from], X[to], (const double*) C[from], C[to], (const int*) P[from], P[to], words );
		if( rc ) return rc;
		}
	return go( k_comb_out, grid, a.audio, ch, n, l.blocks, rounds, local, a.sr, a.cutoff, a.cutoff_c, a.wet_dry, a.wet_dry_c, sign,
		(const double*) X[0], (const double*) X[1], words, a.out );
	}

} // namespace

} // namespace flanhip

using namespace flanhip;

extern "C" {

size_t flanhip_filter_comb_workspace_bytes( int64_t num_channels, int64_t num_frames )
	{
	CombLayout l;
	if( !comb_layout( num_channels, num_frames, &l ) ) return 0;
	return l.total;
	}

void flanhip_filter_comb_debug_local( int rounds )
	{
	t_comb_local = rounds;
	}

int flanhip_filter_comb_dev( const float * d_audio, int64_t num_channels, int64_t num_frames, float sample_rate,
	const float * d_cutoff, float cutoff, const float * d_feedback, float feedback, const float * d_wet_dry, float wet_dry, int invert,
	float * d_out, void * d_workspace, void * stream )
	{
	const CombArgs a{ d_audio, num_channels, num_frames, sample_rate, d_cutoff, cutoff, d_feedback, feedback, d_wet_dry, wet_dry, invert, d_out };
	return launch_comb( a, d_workspace, (hipStream_t) stream );
	}

int flanhip_filter_comb( const float * audio, int64_t num_channels, int64_t num_frames, float sample_rate,
	const float * cutoff_curve, float cutoff, const float * feedback_curve, float feedback, const float * wet_dry_curve, float wet_dry, int invert,
	float * out, volatile int * cancel )
	{
	CombArgs a{ audio, num_channels, num_frames, sample_rate, nullptr, cutoff, nullptr, feedback, nullptr, wet_dry, invert, out };
	CombLayout l;
	if( int rc = comb_check( a, &l ) ) return rc;
	if( int rc = require_device() ) return rc;
	if( cancelled( cancel ) ) return FLANHIP_ERR_CANCELLED;
	const size_t x_bytes = sizeof( float ) * size_t( num_channels ) * size_t( num_frames ), row_bytes = sizeof( float ) * size_t( num_frames );
	HostCall call( cancel );
	void * d_ws = nullptr;
	if( int rc = call.in( audio, x_bytes, &a.audio ) ) return rc;
	if( int rc = call.out( out, x_bytes, &a.out ) ) return rc;
	if( int rc = call.scratch( l.total, &d_ws ) ) return rc;
	if( cutoff_curve ) if( int rc = call.in( cutoff_curve, row_bytes, &a.cutoff ) ) return rc;
	if( feedback_curve ) if( int rc = call.in( feedback_curve, row_bytes, &a.feedback ) ) return rc;
	if( wet_dry_curve ) if( int rc = call.in( wet_dry_curve, row_bytes, &a.wet_dry ) ) return rc;
	if( int rc = call.ready() ) return rc;
	if( int rc = launch_comb( a, d_ws, nullptr, cancel ) ) return rc;
	return call.finish();
	}

} // extern "C"
